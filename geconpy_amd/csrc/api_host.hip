// Host twins of the C ABI (include/dsge_hip.h: every *_host entry point): host pointers in, host pointers out.  A twin
// checks its arguments, declares its buffers to a HostCall, calls the device-pointer entry point (dsge_api.hip) on the
// calling thread's stream and copies the outputs back.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "dsge_host.hpp"

using namespace dsge_host;

namespace {

// ---- staging arenas -------------------------------------------------------------------------------------------------------
// Host threads call the twins concurrently (ctypes releases the GIL: PyMC / nutpie chains in threads, two pytensor Ops),
// so a twin LEASES a staging arena for the duration of its call from a pool that grows to the number of concurrent
// callers; arenas are never shared between two calls in flight and never freed while leased.
struct Arena {
  void* ptr = nullptr;
  size_t cap = 0;
  int dev = -1;
  bool leased = false;
};
constexpr int MAX_DEV = 16;
std::mutex g_stage_mutex;
std::vector<Arena*> g_stage_pool;

// One call of a host twin: the calling thread's two streams, the leased arena and the list of buffers the call stages.
//
//   HostCall hc;
//   if ((rc = hc.begin())) return rc;            // device check, streams
//   hc.in(&dA, A, nn); hc.out(&dT, T_out, nn);   // one line per buffer; a null host pointer declares nothing (dX = nullptr)
//   if ((rc = hc.stage())) return rc;            // sizes and leases the arena, fills dA, dT, ..., enqueues the uploads
//   if ((rc = dsge_..._batched(dA, ..., dT, hc.stream()))) return rc;
//   return hc.finish();                          // enqueues the downloads, synchronises
//
// The arena is sized from the declared list, so it cannot be smaller than what the list carves.  A call that leaves
// between stage() and the end of finish() (a refusal of the device entry such as DSGE_ERR_TOO_LARGE, a HIP error) has
// copies or kernels in flight on the thread's streams: the destructor waits for them BEFORE it gives the arena back,
// since another host thread may lease it at once.
class HostCall {
 public:
  HostCall() = default;
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  ~HostCall() {
    if (pending_) {  // first: nothing of this call may still touch the arena ...
      for (hipStream_t s : s_) (void)hipStreamSynchronize(s);
      (void)hipGetLastError();  // (clear the sticky error, as HIP_TRY does)
    }
    if (arena_) {  // ... then: the arena is free for the next caller
      std::lock_guard<std::mutex> lk(g_stage_mutex);
      arena_->leased = false;
    }
  }

  int begin() {
    int rc = ensure_device();
    if (rc) return rc;
    return twin_streams(&s_[0], &s_[1]);
  }
  hipStream_t stream(int i = 0) const { return s_[i]; }

  // Declarations, in the order the arena is carved.  *dev is null at once for a null host pointer and the device address
  // after stage() otherwise.
  template <typename T>
  void in(const T** dev, const T* host, size_t count) {  // uploaded by stage()
    declare(dev, host, host, nullptr, count * sizeof(T));
  }
  template <typename T>
  void out(T** dev, T* host, size_t count) {  // downloaded by finish()
    declare(dev, host, nullptr, host, count * sizeof(T));
  }
  template <typename T>
  void io(T** dev, T* host, size_t count) {  // both
    declare(dev, host, host, host, count * sizeof(T));
  }
  template <typename T>
  void space(T** dev, size_t count) {  // device space only: the caller copies, or nobody does
    declare(dev, dev, nullptr, nullptr, count * sizeof(T));
  }

  // The observation model / the shock covariance of a filter call on `batch` draws of a model with m variables / k shocks: the host
  // arrays of `host` as inputs, *dev the same description with the device addresses after stage().  upload = false: a per-draw
  // member gets its space only (the caller uploads it chunk by chunk).
  void in(ObsModel* dev, const ObsModel& host, int batch, int m, bool upload = true) {
    *dev = host;
    const size_t b = (size_t)batch, p = (size_t)host.p;
    member(&dev->Z, host.Z, (host.z_batched ? b : 1) * p * m, upload || !host.z_batched);
    member(&dev->d, host.d, (host.d_batched ? b : 1) * p, upload || !host.d_batched);
    member(&dev->Hdiag, host.Hdiag, (host.h_batched ? b : 1) * p, upload || !host.h_batched);
    in(&dev->y, host.y, (size_t)host.T_len * p);
  }
  void in(ShockCov* dev, const ShockCov& host, int batch, int k, bool upload = true) {
    *dev = host;
    member(&dev->Q, host.Q, host.elems(batch, k), upload || !host.batched());
  }
  // The ten inputs of a filter problem across dated breaks: every per-draw array carries the segment axis behind the draw axis, so
  // they are staged as batch * S "draws" (the shared ones as S).  seg_start stays the HOST list.
  void in(SegmentedProblem* dev, const SegmentedProblem& host) {
    *dev = host;
    const ObsModel& o = host.obs;
    const size_t b = (size_t)host.batch, S = (size_t)host.n_seg, flat = host.flat(), m = (size_t)host.m, mm = m * m, p = (size_t)o.p;
    in(&dev->T, host.T, flat * mm);
    in(&dev->R, host.R, flat * m * host.k);
    in(&dev->q.Q, host.q.Q, (host.q.batched() ? flat : S) * host.q_width());
    in(&dev->obs.Z, o.Z, (o.z_batched ? flat : S) * p * m);
    in(&dev->obs.d, o.d, (o.d_batched ? flat : S) * p);
    in(&dev->obs.Hdiag, o.Hdiag, (o.h_batched ? flat : S) * p);
    in(&dev->a0, host.a0, b * m);
    in(&dev->P0, host.P0, b * mm);
    in(&dev->shift, host.shift, flat * m);
    in(&dev->obs.y, o.y, (size_t)o.T_len * p);
  }

  // Ends the declarations: leases an arena that holds every declared buffer (each rounded up to 256 bytes), assigns the
  // addresses in declaration order and enqueues the uploads on stream 0.
  int stage() {
    size_t bytes = TAIL_PAD;
    for (const Buf& b : bufs_) bytes += align256(b.bytes);
    void* base = nullptr;
    int rc = lease(bytes, &base);
    if (rc) return rc;
    pending_ = true;
    size_t off = 0;
    for (const Buf& b : bufs_) {
      void* p = (char*)base + off;
      off += align256(b.bytes);
      std::memcpy(b.slot, &p, sizeof p);  // (the caller's typed pointer)
      if (b.up) HIP_TRY(hipMemcpyAsync(p, b.up, b.bytes, hipMemcpyHostToDevice, s_[0]));
    }
    return DSGE_SUCCESS;
  }

  // After the device entry: every declared output back on stream 0, then wait for it.
  int finish() {
    for (const Buf& b : bufs_)
      if (b.down) {
        void* p = nullptr;
        std::memcpy(&p, b.slot, sizeof p);
        HIP_TRY(hipMemcpyAsync(b.down, p, b.bytes, hipMemcpyDeviceToHost, s_[0]));
      }
    HIP_TRY(hipStreamSynchronize(s_[0]));
    pending_ = false;
    return DSGE_SUCCESS;
  }

 private:
  struct Buf {
    void* slot;  // address of the caller's device pointer
    const void* up;
    void* down;
    size_t bytes;
  };
  // Added to every total.  The hand-counted totals this class replaced carried undocumented slack of 4096, 8192 or 16384
  // bytes depending on the twin (and + 8 / + 64 inside some terms); whether a kernel reads a few bytes past its last
  // input was never established, so the largest of them stays behind the last buffer of every call.
  static constexpr size_t TAIL_PAD = 16384;
  static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

  void member(const double** dev, const double* host, size_t count, bool upload) {
    declare(dev, host, upload ? host : nullptr, nullptr, count * sizeof(double));
  }
  template <typename P>
  void declare(P** dev, const void* present, const void* up, void* down, size_t bytes) {
    *dev = nullptr;
    if (present) bufs_.push_back(Buf{(void*)dev, up, down, bytes});
  }

  int lease(size_t bytes, void** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEV) return fail(DSGE_ERR_INVALID, "device index out of range");
    Arena* a = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_stage_mutex);
      for (Arena* c : g_stage_pool)  // the largest free arena of this device
        if (!c->leased && c->dev == dev && (!a || c->cap > a->cap)) a = c;
      if (!a) {
        a = new Arena();
        a->dev = dev;
        g_stage_pool.push_back(a);
      }
      a->leased = true;
    }
    arena_ = a;
    if (a->cap < bytes) {  // only this call holds the arena: nothing of it is in flight
      if (a->ptr) {
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

  hipStream_t s_[2] = {nullptr, nullptr};
  Arena* arena_ = nullptr;
  bool pending_ = false;  // staged, and finish() has not synchronised yet
  std::vector<Buf> bufs_;
};

int cr_host(const double* A, const double* B, const double* C, int batch, int n, int max_iter, double tol, double* T_out,
            int32_t* status, int32_t* n_iter, int scan_mode) {
  int rc = check_common(batch, n, DSGE_MAX_N_BIG);
  if (rc) return rc;
  if (!A || !B || !C || !T_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n;
  const double *dA, *dB, *dC;
  double* dT;
  int32_t *dS, *dI;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.out(&dT, T_out, nn);
  hc.out(&dS, status, batch);
  hc.out(&dI, n_iter, batch);
  if ((rc = hc.stage())) return rc;
  rc = scan_mode ? dsge_scan_cycle_reduction_batched(dA, dB, dC, batch, n, max_iter, tol, dT, dS, dI, hc.stream())
                 : dsge_cycle_reduction_batched(dA, dB, dC, batch, n, max_iter, tol, dT, dS, dI, hc.stream());
  if (rc) return rc;
  return hc.finish();
}

// the two gradient twins: dense_z selects the entry point with the design matrix's adjoint (Z_bar, optional)
int grad_host(const double* A, const double* B, const double* C, const double* D, const double* q, int q_batched,
              const double* Z, int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
              const double* y, int batch, int n, int k, int p, int T_len, int solver, double tol, int max_iter, double jitter,
              double missing_fill, int n_filter_hint, int n_lead_hint, double* logp_out, int32_t* status_out, double* A_bar,
              double* B_bar, double* C_bar, double* D_bar, double* q_bar, double* d_bar, double* h_bar, bool dense_z,
              double* Z_bar) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov qc{q, q_batched};
  int rc = check_grad(batch, n, k, obs, qc, solver, dense_z,
                      A && B && C && D && logp_out && status_out && A_bar && B_bar && C_bar && D_bar && q_bar);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k, bp = (size_t)batch * p;
  ObsModel dobs;
  ShockCov dq;
  const double *dA, *dB, *dC, *dD;
  double *dL, *gA, *gB, *gC, *gD, *gq, *gd, *gh, *gZ;
  int32_t* dS;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, D, nk);
  hc.in(&dq, qc, batch, k);
  hc.in(&dobs, obs, batch, n);
  hc.out(&dL, logp_out, batch);
  hc.out(&dS, status_out, batch);
  hc.out(&gA, A_bar, nn);
  hc.out(&gB, B_bar, nn);
  hc.out(&gC, C_bar, nn);
  hc.out(&gD, D_bar, nk);
  hc.out(&gq, q_bar, (size_t)batch * qc.elems(1, k));
  hc.out(&gd, d_bar, bp);
  hc.out(&gh, h_bar, bp);
  hc.out(&gZ, dense_z ? Z_bar : nullptr, (size_t)batch * p * n);
  if ((rc = hc.stage())) return rc;
  rc = dense_z ? dsge_solve_kalman_logp_grad_dense_z_batched(dA, dB, dC, dD, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d,
                                                             dobs.d_batched, dobs.Hdiag, dobs.h_batched, dobs.y, batch, n, k, p, T_len, solver, tol,
                                                             max_iter, jitter, missing_fill, n_filter_hint, n_lead_hint, dL, dS, gA, gB,
                                                             gC, gD, gq, gd, gh, gZ, hc.stream())
               : dsge_solve_kalman_logp_grad_batched(dA, dB, dC, dD, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched,
                                                     dobs.Hdiag, dobs.h_batched, dobs.y, batch, n, k, p, T_len, solver, tol,
                                                     max_iter, jitter, missing_fill, n_filter_hint, n_lead_hint, dL, dS, gA, gB, gC, gD, gq,
                                                     gd, gh, hc.stream());
  if (rc) return rc;
  return hc.finish();
}

}  // namespace

extern "C" {

int dsge_cycle_reduction_batched_host(const double* A, const double* B, const double* C, int batch, int n,
                                      int max_iter, double tol, double* T_out, int32_t* status, int32_t* n_iter) {
  return cr_host(A, B, C, batch, n, max_iter, tol, T_out, status, n_iter, 0);
}

int dsge_scan_cycle_reduction_batched_host(const double* A, const double* B, const double* C, int batch, int n,
                                           int max_iter, double tol, double* T_out, int32_t* status,
                                           int32_t* n_steps) {
  return cr_host(A, B, C, batch, n, max_iter, tol, T_out, status, n_steps, 1);
}

int dsge_gensys_batched_host(const double* A, const double* B, const double* C, const double* D, int batch, int n,
                             int k, double tol, int n_lead_hint, double* T_out, double* R_out, int32_t* eu_out,
                             int32_t* status) {
  int rc = check_common(batch, n, (big_size(n) && opt().gensys_doubling != 0) ? DSGE_MAX_N_BIG : DSGE_MAX_N_GENSYS - 1);
  if (rc) return rc;
  if (!A || !B || !C || !T_out || !eu_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if (R_out && (!D || k < 1 || k > n)) return fail(DSGE_ERR_INVALID, "R_out requires D and 1 <= k <= n");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * (R_out ? k : 0);
  const double *dA, *dB, *dC, *dD;
  double *dT, *dR;
  int32_t *dE, *dS;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, R_out ? D : nullptr, nk);  // (D is read for R_out only)
  hc.out(&dT, T_out, nn);
  hc.out(&dR, R_out, nk);
  hc.out(&dE, eu_out, (size_t)batch * 3);
  hc.out(&dS, status, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_gensys_batched(dA, dB, dC, dD, batch, n, k, tol, n_lead_hint, dT, dR, dE, dS, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_gensys_pencil_batched_host(const double* g0, const double* g1, const double* c, const double* psi, const double* pi,
                                    int batch, int N, int k, int n_eta, double tol, double* G1_out, double* C_out,
                                    double* impact_out, double* gev_out, int32_t* eu_out, int32_t* status) {
  return dsge_gensys_pencil_full_batched_host(g0, g1, c, psi, pi, batch, N, k, n_eta, tol, G1_out, C_out, impact_out, gev_out,
                                              eu_out, status, nullptr);
}

int dsge_gensys_pencil_full_batched_host(const double* g0, const double* g1, const double* c, const double* psi,
                                         const double* pi, int batch, int N, int k, int n_eta, double tol, double* G1_out,
                                         double* C_out, double* impact_out, double* gev_out, int32_t* eu_out,
                                         int32_t* status, const dsge_gensys_forward* forward) {
  int rc = check_common(batch, N, DSGE_MAX_N_GENSYS);
  if (rc) return rc;
  if (k < 1 || n_eta < 0 || n_eta + k + 1 > 64) return fail(DSGE_ERR_INVALID, "need k >= 1, n_eta >= 0, n_eta + k + 1 <= 64");
  if (!g0 || !g1 || !psi || (n_eta > 0 && !pi) || !G1_out || !C_out || !impact_out || !gev_out || !eu_out || !status)
    return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * N * N, nk = (size_t)batch * N * k, ne = (size_t)batch * N * (n_eta > 0 ? n_eta : 1),
               nv = (size_t)batch * N;
  const dsge_gensys_forward fh = forward ? *forward : dsge_gensys_forward{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  const double *d0, *d1, *dc, *dps, *dpi;
  double *dG, *dC, *dI, *dV;
  int32_t *dE, *dS;
  dsge_gensys_forward fd{nullptr, nullptr, nullptr, nullptr, nullptr, fh.pi_raw};  // the same struct of device pointers
  hc.in(&d0, g0, nn);
  hc.in(&d1, g1, nn);
  hc.in(&dc, c, nv);
  hc.in(&dps, psi, nk);
  hc.in(&dpi, pi, (size_t)batch * N * n_eta);
  hc.out(&dG, G1_out, nn);
  hc.out(&dC, C_out, nv);
  hc.out(&dI, impact_out, nk);
  hc.out(&dV, gev_out, nv * 4);
  hc.out(&dE, eu_out, (size_t)batch * 3);
  hc.out(&dS, status, batch);
  hc.out(&fd.f_mat, fh.f_mat, nn * 2);
  hc.out(&fd.f_wt, fh.f_wt, nk * 2);
  hc.out(&fd.y_wt, fh.y_wt, nn * 2);
  hc.out(&fd.loose, fh.loose, ne);
  hc.out(&fd.n_unstable, fh.n_unstable, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_gensys_pencil_full_batched(d0, d1, dc, dps, dpi, batch, N, k, n_eta, tol, dG, dC, dI, dV, dE, dS,
                                            forward ? &fd : nullptr, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_bk_eigenvalues_batched_host(const double* A, const double* B, const double* C, int batch, int n, double tol,
                                     double* eig_re, double* eig_im, int32_t* n_eig, int32_t* n_forward,
                                     int32_t* n_unstable, int32_t* status) {
  int rc = check_common(batch, n, DSGE_MAX_N_GENSYS - 1);
  if (rc) return rc;
  if (!A || !B || !C || !eig_re || !eig_im || !n_eig || !n_forward || !n_unstable || !status)
    return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, ne = (size_t)batch * 2 * n;
  const double *dA, *dB, *dC;
  double *dRe, *dIm;
  int32_t *dNe, *dNf, *dNu, *dS;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.out(&dRe, eig_re, ne);
  hc.out(&dIm, eig_im, ne);
  hc.out(&dNe, n_eig, batch);
  hc.out(&dNf, n_forward, batch);
  hc.out(&dNu, n_unstable, batch);
  hc.out(&dS, status, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_bk_eigenvalues_batched(dA, dB, dC, batch, n, tol, dRe, dIm, dNe, dNf, dNu, dS, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_selection_batched_host(const double* A, const double* B, const double* C, const double* D, const double* T,
                                int batch, int n, int k, double* R_out, double* resid_out) {
  int rc = check_common(batch, n, DSGE_MAX_N_BIG);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!B || !C || !D || !T || !R_out) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  const double *dA, *dB, *dC, *dD, *dT;
  double *dR, *dRes;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, D, nk);
  hc.in(&dT, T, nn);
  hc.out(&dR, R_out, nk);
  hc.out(&dRes, resid_out, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_selection_batched(dA, dB, dC, dD, dT, batch, n, k, dR, dRes, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_selection_adjoints_batched_host(const double* B, const double* C, const double* T, const double* R,
                                         const double* R_bar, int batch, int n, int k, double* B_bar, double* C_bar,
                                         double* D_bar, double* T_bar) {
  int rc = check_common(batch, n, 56);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!B || !C || !T || !R || !R_bar || !B_bar || !C_bar || !D_bar || !T_bar) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  const double *dB, *dC, *dT, *dR, *dRb;
  double *dBb, *dCb, *dDb, *dTb;
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dT, T, nn);
  hc.in(&dR, R, nk);
  hc.in(&dRb, R_bar, nk);
  hc.out(&dBb, B_bar, nn);
  hc.out(&dCb, C_bar, nn);
  hc.out(&dDb, D_bar, nk);
  hc.out(&dTb, T_bar, nn);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_selection_adjoints_batched(dB, dC, dT, dR, dRb, batch, n, k, dBb, dCb, dDb, dTb, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_policy_adjoints_batched_host(const double* B, const double* C, const double* T, const double* T_bar,
                                      int batch, int n, double* A_bar, double* B_bar, double* C_bar, int32_t* status) {
  int rc = check_common(batch, n, 56);
  if (rc) return rc;
  if (!B || !C || !T || !T_bar || !A_bar || !B_bar || !C_bar || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n;
  const double *dB, *dC, *dT, *dTb;
  double *dAb, *dBb, *dCb;
  int32_t* dS;
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dT, T, nn);
  hc.in(&dTb, T_bar, nn);
  hc.out(&dAb, A_bar, nn);
  hc.out(&dBb, B_bar, nn);
  hc.out(&dCb, C_bar, nn);
  hc.out(&dS, status, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_policy_adjoints_batched(dB, dC, dT, dTb, batch, n, dAb, dBb, dCb, dS, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_second_order_logp_batched_host(const double* A, const double* B, const double* C, const double* D,
                                        const int32_t* hess_idx, int nnz, const double* hess_val, const double* q,
                                        int q_batched, const double* Z, const double* d, const double* Hdiag, const double* y,
                                        int batch, int n, int k, int p, int T_len, int solver, double tol, int max_iter,
                                        double jitter, double missing_fill, const int32_t* state_idx, int n_state,
                                        const int32_t* lead_idx, int n_lead, const int32_t* ret_idx, int n_ret,
                                        double* logp_out, int32_t* status_out, double* T_out, double* R_out, double* gyy_out,
                                        double* gyu_out, double* guu_out, double* gss_out) {
  const ObsModel obs{Z, 0, d, 0, Hdiag, 0, y, p, T_len, jitter, missing_fill};
  const ShockCov qc{q, q_batched ? DSGE_Q_DIAG_BATCHED : DSGE_Q_DIAG_SHARED};
  int rc = check_second_order(batch, n, k, obs, qc, solver, nnz, state_idx, n_state, lead_idx, n_lead, ret_idx, n_ret,
                              A && B && C && D && (nnz == 0 || (hess_idx && hess_val)) && logp_out && status_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k, nv = (size_t)batch * nnz, ss = (size_t)n_state * n_state;
  ObsModel dobs;
  ShockCov dq;
  const double *dA, *dB, *dC, *dD, *dHv;
  const int32_t* dHi;
  double *dlp, *dT, *dR, *dgyy, *dgyu, *dguu, *dgss;
  int32_t* dst;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, D, nk);
  hc.in(&dHi, hess_idx, (size_t)nnz * 3);
  hc.in(&dHv, hess_val, nv);
  hc.in(&dq, qc, batch, k);
  hc.in(&dobs, obs, batch, n);
  hc.out(&dlp, logp_out, batch);
  hc.out(&dst, status_out, batch);
  hc.out(&dT, T_out, nn);
  hc.out(&dR, R_out, nk);
  hc.out(&dgyy, gyy_out, (size_t)batch * n * ss);
  hc.out(&dgyu, gyu_out, (size_t)batch * n * n_state * k);
  hc.out(&dguu, guu_out, (size_t)batch * n * k * k);
  hc.out(&dgss, gss_out, (size_t)batch * n);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_second_order_logp_batched(dA, dB, dC, dD, dHi, nnz, dHv, dq.Q, q_batched, dobs.Z, dobs.d, dobs.Hdiag, dobs.y, batch, n, k, p, T_len,
                                           solver, tol, max_iter, jitter, missing_fill, state_idx, n_state, lead_idx, n_lead,
                                           ret_idx, n_ret, dlp, dst, dT, dR, dgyy, dgyu, dguu, dgss, nullptr, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_filter_outputs_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                            int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                            const double* y, int batch, int m, int k, int p, int T_len, double jitter,
                                            double missing_fill, double* ll_out, double* a_pred_out, double* a_filt_out,
                                            double* p_pred_out, double* p_filt_out, int full_cov, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman(batch, m, k, obs, q, T && R && ll_out && status_io);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t mm = (size_t)batch * m * m, mk = (size_t)batch * m * k, tm = (size_t)batch * T_len * m, tc = full_cov ? tm * m : tm;
  ObsModel dobs;
  ShockCov dq;
  const double *dT, *dR;
  double *dll, *dap, *daf, *dpp, *dpf;
  int32_t* dS;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, mk);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.io(&dS, status_io, batch);
  hc.out(&dll, ll_out, (size_t)batch * T_len);
  hc.out(&dap, a_pred_out, tm);
  hc.out(&daf, a_filt_out, tm);
  hc.out(&dpp, p_pred_out, tc);
  hc.out(&dpf, p_filt_out, tc);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_filter_outputs_batched(dT, dR, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched, dobs.Hdiag,
                                               dobs.h_batched, dobs.y, batch, m, k, p, T_len, jitter, missing_fill, dll, dap,
                                               daf, dpp, dpf, full_cov, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_logp_segments_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                           int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                           const double* a0, const double* P0, const double* shift, const double* y,
                                           const int32_t* seg_start, int n_seg, int batch, int m, int k, int p, int T_len,
                                           double jitter, double missing_fill, double* logp_out, double* ll_out, double* a_last_out,
                                           double* P_last_out, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && logp_out && status_io);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  SegmentedProblem ds;
  double *dlp, *dll, *dal, *dpl;
  int32_t* dS;
  hc.in(&ds, SegmentedProblem{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k});
  hc.io(&dS, status_io, (size_t)batch);
  hc.out(&dlp, logp_out, (size_t)batch);
  hc.out(&dll, ll_out, (size_t)batch * T_len);
  hc.out(&dal, a_last_out, (size_t)batch * m);
  hc.out(&dpl, P_last_out, (size_t)batch * m * m);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_logp_segments_batched(ds.T, ds.R, ds.q.Q, q_mode, ds.obs.Z, z_batched, ds.obs.d, d_batched, ds.obs.Hdiag,
                                              h_batched, ds.a0, ds.P0, ds.shift, ds.obs.y, seg_start, n_seg, batch, m, k, p, T_len,
                                              jitter, missing_fill, dlp, dll, dal, dpl, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_smoother_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                      const double* d, int d_batched, const double* Hdiag, int h_batched, const double* y,
                                      int batch, int m, int k, int p, int T_len, double jitter, double missing_fill,
                                      double rank_tol, size_t scratch_limit_bytes, double* ll_out, double* a_smooth_out,
                                      double* p_smooth_out, double* eps_smooth_out, int full_cov, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_smoother(batch, m, k, obs, q, T && R && status_io, a_smooth_out || p_smooth_out || eps_smooth_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  const size_t mm = (size_t)batch * m * m, mk = (size_t)batch * m * k, tm = (size_t)batch * T_len * m, tc = full_cov ? tm * m : tm;
  ObsModel dobs;
  ShockCov dq;
  const double *dT, *dR;
  double *dll, *das, *dps, *des;
  int32_t* dS;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, mk);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.io(&dS, status_io, batch);
  hc.out(&dll, ll_out, (size_t)batch * T_len);
  hc.out(&das, a_smooth_out, tm);
  hc.out(&dps, p_smooth_out, tc);
  hc.out(&des, eps_smooth_out, (size_t)batch * T_len * k);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_smoother_batched(dT, dR, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched, dobs.Hdiag,
                                         dobs.h_batched, dobs.y, batch, m, k, p, T_len,
                                         jitter, missing_fill, rank_tol, scratch_limit_bytes, dll, das, dps, des, full_cov, dS,
                                         hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_smoother_segments_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                               int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                               const double* a0, const double* P0, const double* shift, const double* y,
                                               const int32_t* seg_start, int n_seg, int batch, int m, int k, int p, int T_len,
                                               double jitter, double missing_fill, double rank_tol, size_t scratch_limit_bytes,
                                               int full_cov, double* ll_out, double* a_pred_out, double* a_filt_out,
                                               double* p_pred_out, double* p_filt_out, double* a_smooth_out, double* p_smooth_out,
                                               double* eps_smooth_out, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_smoother_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && status_io,
                                   ll_out || a_pred_out || a_filt_out || p_pred_out || p_filt_out || a_smooth_out || p_smooth_out ||
                                       eps_smooth_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  const size_t tm = (size_t)batch * T_len * m, tc = full_cov ? tm * m : tm;
  SegmentedProblem ds;
  double *dll, *dap, *daf, *dpp, *dpf, *das, *dps, *des;
  int32_t* dS;
  hc.in(&ds, SegmentedProblem{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k});
  hc.io(&dS, status_io, (size_t)batch);
  hc.out(&dll, ll_out, (size_t)batch * T_len);
  hc.out(&dap, a_pred_out, tm);
  hc.out(&daf, a_filt_out, tm);
  hc.out(&dpp, p_pred_out, tc);
  hc.out(&dpf, p_filt_out, tc);
  hc.out(&das, a_smooth_out, tm);
  hc.out(&dps, p_smooth_out, tc);
  hc.out(&des, eps_smooth_out, (size_t)batch * T_len * k);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_smoother_segments_batched(ds.T, ds.R, ds.q.Q, q_mode, ds.obs.Z, z_batched, ds.obs.d, d_batched, ds.obs.Hdiag,
                                                  h_batched, ds.a0, ds.P0, ds.shift, ds.obs.y, seg_start, n_seg, batch, m, k, p,
                                                  T_len, jitter, missing_fill, rank_tol, scratch_limit_bytes, full_cov, dll, dap, daf,
                                                  dpp, dpf, das, dps, des, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_logp_segments_grad_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                                int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                                const double* a0, const double* P0, const double* shift, const double* y,
                                                const int32_t* seg_start, int n_seg, int batch, int m, int k, int p, int T_len,
                                                double jitter, double missing_fill, size_t scratch_limit_bytes, double* logp_out,
                                                double* T_bar, double* R_bar, double* Q_bar, double* Z_bar, double* d_bar,
                                                double* h_bar, double* shift_bar, double* a0_bar, double* P0_bar, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && logp_out && status_io);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  // the cotangents carry the segment axis as the inputs do; Q_bar is per draw in every layout
  const SegmentedProblem hs{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k};
  const size_t flat = hs.flat(), mm = (size_t)m * m, qw = hs.q_width();
  SegmentedProblem ds;
  double *dlp, *dTb, *dRb, *dQb, *dZb, *ddb, *dhb, *dsb, *dab, *dPb;
  int32_t* dS;
  hc.in(&ds, hs);
  hc.io(&dS, status_io, (size_t)batch);
  hc.out(&dlp, logp_out, (size_t)batch);
  hc.out(&dTb, T_bar, flat * mm);
  hc.out(&dRb, R_bar, flat * m * k);
  hc.out(&dQb, Q_bar, flat * qw);
  hc.out(&dZb, Z_bar, flat * p * m);
  hc.out(&ddb, d_bar, flat * p);
  hc.out(&dhb, h_bar, flat * p);
  hc.out(&dsb, shift_bar, flat * m);
  hc.out(&dab, a0_bar, (size_t)batch * m);
  hc.out(&dPb, P0_bar, (size_t)batch * mm);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_logp_segments_grad_batched(ds.T, ds.R, ds.q.Q, q_mode, ds.obs.Z, z_batched, ds.obs.d, d_batched, ds.obs.Hdiag,
                                                   h_batched, ds.a0, ds.P0, ds.shift, ds.obs.y, seg_start, n_seg, batch, m, k, p,
                                                   T_len, jitter, missing_fill, scratch_limit_bytes, dlp, dTb, dRb, dQb, dZb, ddb, dhb,
                                                   dsb, dab, dPb, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_simulation_smoother_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                          const double* d, int d_batched, const double* Hdiag, int h_batched, const double* y,
                                          int batch, int m, int k, int p, int T_len, double jitter, double missing_fill,
                                          double rank_tol, size_t scratch_limit_bytes, const double* x0, int x0_batched,
                                          const double* eps, int eps_batched, const double* eta, int eta_batched, int n_paths,
                                          double* ll_out, double* x_out, double* eps_out, int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_simulation_smoother(batch, m, k, obs, q, T && R && status_io, n_paths, eps, eta, x_out || eps_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || T_len == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, np = (size_t)n_paths, tl = (size_t)T_len;
  ObsModel dobs;
  ShockCov dq;
  const double *dT, *dR, *dx0, *deps, *deta;
  double *dll, *dx, *de;
  int32_t* dS;
  hc.in(&dT, T, b * m * m);
  hc.in(&dR, R, b * m * k);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.in(&dx0, x0, (x0_batched ? b : 1) * np * m);
  hc.in(&deps, eps, (eps_batched ? b : 1) * np * tl * k);
  hc.in(&deta, eta, (eta_batched ? b : 1) * np * tl * p);
  hc.io(&dS, status_io, b);
  hc.out(&dll, ll_out, b * tl);
  hc.out(&dx, x_out, b * np * tl * m);
  hc.out(&de, eps_out, b * np * tl * k);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_simulation_smoother_batched(dT, dR, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched, dobs.Hdiag,
                                             dobs.h_batched, dobs.y, batch, m, k, p, T_len, jitter, missing_fill, rank_tol,
                                             scratch_limit_bytes, dx0, x0_batched, deps, eps_batched, deta, eta_batched, n_paths, dll,
                                             dx, de, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_simulate_batched_host(const double* T, const double* R, const double* eps, int eps_batched, const double* x0,
                               int x0_batched, const int32_t* status, int batch, int m, int k, int n_paths, int n_steps,
                               int n_shock_steps, double* x_out) {
  int rc = check_simulate(T, R, eps, batch, m, k, n_paths, n_steps, n_shock_steps, x_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const double *dT, *dR, *de, *dx0;
  const int32_t* dS;
  double* dx;
  hc.in(&dT, T, (size_t)batch * m * m);
  hc.in(&dR, R, (size_t)batch * m * k);
  hc.in(&de, eps, (size_t)(eps_batched ? batch : 1) * n_paths * n_shock_steps * k);
  hc.in(&dx0, x0, (size_t)(x0_batched ? batch : 1) * n_paths * m);
  hc.in(&dS, status, (size_t)batch);
  hc.out(&dx, x_out, (size_t)batch * n_paths * n_steps * m);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_simulate_batched(dT, dR, de, eps_batched, dx0, x0_batched, dS, batch, m, k, n_paths, n_steps, n_shock_steps, dx,
                                  hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_irf_batched_host(const double* T, const double* R, const double* S, int s_batched, const double* weights, int w_batched,
                          const int32_t* status, int batch, int m, int k, int c, int n_steps, double* irf_out, double* fevd_out) {
  int rc = check_irf(T, R, S, batch, m, k, c, n_steps, irf_out, fevd_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || c == 0 || n_steps == 0) return DSGE_SUCCESS;
  const double *dT, *dR, *dSm, *dw;
  const int32_t* dS;
  double *di, *df;
  const size_t no = (size_t)batch * c * n_steps * m;
  hc.in(&dT, T, (size_t)batch * m * m);
  hc.in(&dR, R, (size_t)batch * m * k);
  hc.in(&dSm, S, (size_t)(s_batched ? batch : 1) * k * c);
  hc.in(&dw, weights, (size_t)(w_batched ? batch : 1) * c);
  hc.in(&dS, status, (size_t)batch);
  hc.out(&di, irf_out, no);
  hc.out(&df, fevd_out, no);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_irf_batched(dT, dR, dSm, s_batched, dw, w_batched, dS, batch, m, k, c, n_steps, di, df, hc.stream()))) return rc;
  return hc.finish();
}

// (state_idx is a host array in the device entries too: it is not staged)
int dsge_simulate_pruned_batched_host(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu,
                                      const double* gss, const int32_t* state_idx, int n_state, const double* eps, int eps_batched,
                                      const double* xf0, const double* xs0, int x0_batched, const int32_t* status, int batch, int n,
                                      int k, int n_paths, int n_steps, int n_shock_steps, double* x_out, double* xf_out,
                                      double* xs_out) {
  int rc = check_pruned(T, R, gyy, gyu, guu, gss, state_idx, n_state, eps, batch, n, k, n_paths, n_steps, n_shock_steps,
                        x_out || xf_out || xs_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, s = (size_t)n_state, no = b * n_paths * n_steps * n, nx = (size_t)(x0_batched ? batch : 1) * n_paths * n;
  const double *dT, *dR, *dyy, *dyu, *duu, *dss, *de, *df0, *ds0;
  const int32_t* dS;
  double *dx, *dxf, *dxs;
  hc.in(&dT, T, b * n * n);
  hc.in(&dR, R, b * n * k);
  hc.in(&dyy, gyy, b * n * s * s);
  hc.in(&dyu, gyu, b * n * s * k);
  hc.in(&duu, guu, b * n * k * k);
  hc.in(&dss, gss, b * n);
  hc.in(&de, eps, (size_t)(eps_batched ? batch : 1) * n_paths * n_shock_steps * k);
  hc.in(&df0, xf0, nx);
  hc.in(&ds0, xs0, nx);
  hc.in(&dS, status, b);
  hc.out(&dx, x_out, no);
  hc.out(&dxf, xf_out, no);
  hc.out(&dxs, xs_out, no);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_simulate_pruned_batched(dT, dR, dyy, dyu, duu, dss, state_idx, n_state, de, eps_batched, df0, ds0, x0_batched, dS, batch,
                                         n, k, n_paths, n_steps, n_shock_steps, dx, dxf, dxs, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_girf_pruned_batched_host(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu,
                                  const double* gss, const int32_t* state_idx, int n_state, const double* S_imp, int s_batched, int c,
                                  const double* eps, int eps_batched, const double* xf0, const double* xs0, int x0_batched,
                                  const int32_t* status, int batch, int n, int k, int n_paths, int n_steps, int n_shock_steps,
                                  double* girf_out) {
  int rc = check_girf_pruned(T, R, gyy, gyu, guu, gss, state_idx, n_state, S_imp, c, eps, batch, n, k, n_paths, n_steps, n_shock_steps,
                             girf_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || c == 0 || n_steps == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, s = (size_t)n_state, nx = (size_t)(x0_batched ? batch : 1) * n_paths * n;
  const double *dT, *dR, *dyy, *dyu, *duu, *dss, *dimp, *de, *df0, *ds0;
  const int32_t* dS;
  double* dg;
  hc.in(&dT, T, b * n * n);
  hc.in(&dR, R, b * n * k);
  hc.in(&dyy, gyy, b * n * s * s);
  hc.in(&dyu, gyu, b * n * s * k);
  hc.in(&duu, guu, b * n * k * k);
  hc.in(&dss, gss, b * n);
  hc.in(&dimp, S_imp, (size_t)(s_batched ? batch : 1) * k * c);
  hc.in(&de, eps, (size_t)(eps_batched ? batch : 1) * n_paths * n_shock_steps * k);
  hc.in(&df0, xf0, nx);
  hc.in(&ds0, xs0, nx);
  hc.in(&dS, status, b);
  hc.out(&dg, girf_out, b * c * n_steps * n);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_girf_pruned_batched(dT, dR, dyy, dyu, duu, dss, state_idx, n_state, dimp, s_batched, c, de, eps_batched, df0, ds0,
                                     x0_batched, dS, batch, n, k, n_paths, n_steps, n_shock_steps, dg, hc.stream())))
    return rc;
  return hc.finish();
}

// (group_of_shock and var_idx are host arrays in the device entry too: they are not staged)
int dsge_shock_decomposition_batched_host(const double* T, const double* R, const double* eps, const double* x,
                                          const int32_t* group_of_shock, int n_groups, const int32_t* var_idx, int n_out,
                                          const double* Z, int z_batched, const int32_t* status, int batch, int m, int k, int p,
                                          int n_paths, int T_len, int remainder, double* contrib_out, double* obs_out) {
  int rc = check_shock_decomp(T, R, eps, x, group_of_shock, n_groups, var_idx, n_out, Z, batch, m, k, p, n_paths, T_len, remainder,
                              contrib_out, obs_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, steps = b * n_paths * T_len, C = (size_t)n_groups + 1 + (remainder ? 1 : 0);
  const double *dT, *dR, *de, *dx, *dZ;
  const int32_t* dS;
  double *dc, *dobs;
  hc.in(&dT, T, b * m * m);
  hc.in(&dR, R, b * m * k);
  hc.in(&de, eps, steps * k);
  hc.in(&dx, x, steps * m);
  hc.in(&dZ, Z, (size_t)(z_batched ? batch : 1) * (Z ? p : 0) * m);
  hc.in(&dS, status, b);
  hc.out(&dc, contrib_out, steps * n_out * C);
  hc.out(&dobs, obs_out, steps * (Z ? p : 0) * C);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_shock_decomposition_batched(dT, dR, de, dx, group_of_shock, n_groups, var_idx, n_out, dZ, z_batched, dS, batch, m, k, p,
                                             n_paths, T_len, remainder, dc, dobs, hc.stream())))
    return rc;
  return hc.finish();
}

// (cond_t, cond_j and free_shock are host arrays in the device entry too: they are not staged)
int dsge_conditional_forecast_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                           int z_batched, const double* d, int d_batched, const double* x0, int x0_batched,
                                           int x0_paths, const double* eps, int eps_batched, const int32_t* cond_t,
                                           const int32_t* cond_j, int n_cond, const double* cond_val, int cv_batched, int cv_paths,
                                           const int32_t* free_shock, int32_t* status_io, int batch, int m, int k, int p,
                                           int n_paths, int n_steps, int n_shock_steps, double rank_tol, double* x_out,
                                           double* eps_out, double* obs_out) {
  CondFcProblem c{batch, m, k, p, n_paths, n_steps, n_shock_steps, n_cond, x0_batched, x0_paths, eps_batched, cv_batched, cv_paths,
                  cond_t, cond_j, free_shock, rank_tol};
  const ShockCov q{Q, q_mode};
  int rc = check_conditional_forecast(c, T, R, q, Z, x0, eps, cond_val, x_out, eps_out, obs_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, np = (size_t)n_paths, ns = (size_t)n_steps;
  ShockCov dq;
  const double *dT, *dR, *dZ, *dd, *dx0, *de, *dcv;
  double *dx, *deo, *dobs;
  int32_t* dS;
  hc.in(&dT, T, b * m * m);
  hc.in(&dR, R, b * m * k);
  hc.in(&dq, q, batch, k);
  hc.in(&dZ, Z, (z_batched ? b : 1) * p * m);
  hc.in(&dd, d, (d_batched ? b : 1) * p);
  hc.in(&dx0, x0, (x0_batched ? b : 1) * (x0_paths ? np : 1) * m);
  hc.in(&de, eps, (eps_batched ? b : 1) * np * n_shock_steps * k);
  hc.in(&dcv, n_cond > 0 ? cond_val : nullptr, (cv_batched ? b : 1) * (cv_paths ? np : 1) * n_cond);
  hc.io(&dS, status_io, b);
  hc.out(&dx, x_out, b * np * ns * m);
  hc.out(&deo, eps_out, b * np * ns * k);
  hc.out(&dobs, obs_out, b * np * ns * p);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_conditional_forecast_batched(dT, dR, dq.Q, dq.mode, dZ, z_batched, dd, d_batched, dx0, x0_batched, x0_paths, de,
                                              eps_batched, cond_t, cond_j, n_cond, dcv, cv_batched, cv_paths, free_shock, dS, batch,
                                              m, k, p, n_paths, n_steps, n_shock_steps, rank_tol, dx, deo, dobs, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_spectral_moments_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                       const double* Hdiag, int h_batched, const double* gain, int batch, int m, int k, int p,
                                       int n_grid, int n_lags, int correlation, double rank_tol, size_t scratch_limit_bytes,
                                       double* acov_out, double* spectrum_out, int32_t* status_io) {
  const SpectralProblem s{batch, m, k, p, n_grid, n_lags, correlation, z_batched, h_batched, rank_tol};
  const ShockCov q{Q, q_mode};
  int rc = check_spectral_moments(s, T, R, q, Z, Hdiag, acov_out, spectrum_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, dim = Z ? p : m, nf = (size_t)n_grid / 2 + 1;
  ShockCov dq;
  const double *dT, *dR, *dZ, *dH, *dg;
  double *dacov, *dspec;
  int32_t* dS;
  hc.in(&dT, T, b * m * m);
  hc.in(&dR, R, b * m * k);
  hc.in(&dq, q, batch, k);
  hc.in(&dZ, Z, (z_batched ? b : 1) * p * m);
  hc.in(&dH, Hdiag, (h_batched ? b : 1) * p);
  hc.in(&dg, gain, nf);
  hc.io(&dS, status_io, b);
  hc.out(&dacov, acov_out, b * (n_lags + 1) * dim * dim);
  hc.out(&dspec, spectrum_out, b * nf * dim * dim * 2);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_spectral_moments_batched(dT, dR, dq.Q, dq.mode, dZ, z_batched, dH, h_batched, dg, batch, m, k, p, n_grid, n_lags,
                                          correlation, rank_tol, scratch_limit_bytes, dacov, dspec, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_anticipated_paths_batched_host(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                        int eps_batched, int mode, int n_lead, const double* x0, int x0_batched, int x0_paths,
                                        const double* Z, int z_batched, const double* d, int d_batched, int32_t* status_io,
                                        int batch, int n, int k, int p, int n_paths, int n_steps, int n_shock_steps,
                                        double rank_tol, double* x_out, double* w_out, double* obs_out, double* G_out) {
  const AnticipatedProblem c{batch, n, k, p, n_paths, n_steps, n_shock_steps, mode, n_lead, eps_batched, x0_batched, x0_paths,
                             z_batched, d_batched, rank_tol};
  int rc = check_anticipated_paths(c, B, C, T, R, eps, Z, x_out, w_out, obs_out, G_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, np = (size_t)n_paths, ns = (size_t)n_steps, nn = (size_t)n * n;
  const size_t rows = (size_t)n_shock_steps * (mode == DSGE_ANT_NEWS ? n_lead + 1 : 1);
  const double *dB, *dC, *dT, *dR, *de, *dx0, *dZ, *dd;
  double *dx, *dw, *dobs, *dG;
  int32_t* dS;
  hc.in(&dB, B, b * nn);
  hc.in(&dC, C, b * nn);
  hc.in(&dT, T, b * nn);
  hc.in(&dR, R, b * n * k);
  hc.in(&de, eps, (eps_batched ? b : 1) * np * rows * k);
  hc.in(&dx0, x0, (x0_batched ? b : 1) * (x0_paths ? np : 1) * n);
  hc.in(&dZ, Z, (z_batched ? b : 1) * p * n);
  hc.in(&dd, d, (d_batched ? b : 1) * p);
  hc.io(&dS, status_io, b);
  hc.out(&dx, x_out, b * np * ns * n);
  hc.out(&dw, w_out, b * np * ns * n);
  hc.out(&dobs, obs_out, b * np * ns * p);
  hc.out(&dG, G_out, b * nn);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_anticipated_paths_batched(dB, dC, dT, dR, de, eps_batched, mode, n_lead, dx0, x0_batched, x0_paths, dZ, z_batched,
                                           dd, d_batched, dS, batch, n, k, p, n_paths, n_steps, n_shock_steps, rank_tol, dx, dw,
                                           dobs, dG, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_constrained_paths_batched_host(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                        int eps_batched, const double* x0, int x0_batched, int x0_paths, const double* Z,
                                        int z_batched, const double* d, int d_batched, const double* c_row, int c_batched,
                                        const double* bound, int bound_batched, int shock, int horizon, int max_iter,
                                        int32_t* status_io, int batch, int n, int k, int p, int n_paths, int n_steps, int n_shock_steps,
                                        double rank_tol, double* x_out, double* w_out, double* obs_out, double* nu_out, double* gap_out,
                                        double* Mz_out, int32_t* path_status_out, int32_t* iters_out) {
  const ConstrainedProblem c{{batch, n, k, p, n_paths, n_steps, n_shock_steps, DSGE_ANT_PERFECT_FORESIGHT, 0, eps_batched, x0_batched,
                              x0_paths, z_batched, d_batched, rank_tol},
                             c_batched, bound_batched, shock, horizon, max_iter};
  const void* other = nu_out ? (const void*)nu_out : gap_out ? (const void*)gap_out : Mz_out ? (const void*)Mz_out
                      : path_status_out ? (const void*)path_status_out : (const void*)iters_out;
  int rc = check_constrained_paths(c, B, C, T, R, eps, Z, c_row, bound, x_out, w_out, obs_out, other);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, np = (size_t)n_paths, ns = (size_t)n_steps, nn = (size_t)n * n, H = (size_t)horizon;
  const double *dB, *dC, *dT, *dR, *de, *dx0, *dZ, *dd, *dc, *dbound;
  double *dx, *dw, *dobs, *dnu, *dgap, *dMz;
  int32_t *dS, *dps, *dit;
  hc.in(&dB, B, b * nn);
  hc.in(&dC, C, b * nn);
  hc.in(&dT, T, b * nn);
  hc.in(&dR, R, b * n * k);
  hc.in(&de, eps, (eps_batched ? b : 1) * np * n_shock_steps * k);
  hc.in(&dx0, x0, (x0_batched ? b : 1) * (x0_paths ? np : 1) * n);
  hc.in(&dZ, Z, (z_batched ? b : 1) * p * n);
  hc.in(&dd, d, (d_batched ? b : 1) * p);
  hc.in(&dc, c_row, (c_batched ? b : 1) * n);
  hc.in(&dbound, bound, bound_batched ? b : 1);
  hc.io(&dS, status_io, b);
  hc.out(&dx, x_out, b * np * ns * n);
  hc.out(&dw, w_out, b * np * ns * n);
  hc.out(&dobs, obs_out, b * np * ns * p);
  hc.out(&dnu, nu_out, b * np * H);
  hc.out(&dgap, gap_out, b * np * ns);
  hc.out(&dMz, Mz_out, b * H * H);
  hc.out(&dps, path_status_out, b * np);
  hc.out(&dit, iters_out, b * np);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_constrained_paths_batched(dB, dC, dT, dR, de, eps_batched, dx0, x0_batched, x0_paths, dZ, z_batched, dd, d_batched, dc,
                                           c_batched, dbound, bound_batched, shock, horizon, max_iter, dS, batch, n, k, p, n_paths,
                                           n_steps, n_shock_steps, rank_tol, dx, dw, dobs, dnu, dgap, dMz, dps, dit, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_constrained_simulate_batched_host(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                           int eps_batched, const double* x0, int x0_batched, int x0_paths, const double* Z,
                                           int z_batched, const double* d, int d_batched, const double* c_row, int c_batched,
                                           const double* bound, int bound_batched, int shock, int horizon, int max_iter,
                                           int32_t* status_io, int batch, int n, int k, int p, int n_paths, int n_steps,
                                           int n_shock_steps, double rank_tol, double* x_out, double* obs_out, double* gap_out,
                                           double* shadow_out, double* plan_out, int32_t* duration_out, int32_t* iters_out,
                                           double* Mz_out, int32_t* path_status_out, int32_t* fail_step_out) {
  const ConstrainedProblem c{{batch, n, k, p, n_paths, n_steps, n_shock_steps, DSGE_ANT_PERFECT_FORESIGHT, 0, eps_batched, x0_batched,
                              x0_paths, z_batched, d_batched, rank_tol},
                             c_batched, bound_batched, shock, horizon, max_iter};
  const void* outs[] = {gap_out, shadow_out, plan_out, duration_out, iters_out, Mz_out, path_status_out, fail_step_out};
  const void* other = nullptr;
  for (const void* o : outs) other = other ? other : o;
  int rc = check_constrained_simulate(c, B, C, T, R, eps, Z, c_row, bound, x_out, obs_out, other);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const size_t b = (size_t)batch, np = (size_t)n_paths, ns = (size_t)n_steps, nn = (size_t)n * n, H = (size_t)horizon;
  const double *dB, *dC, *dT, *dR, *de, *dx0, *dZ, *dd, *dc, *dbound;
  double *dx, *dobs, *dgap, *dsh, *dplan, *dMz;
  int32_t *dS, *ddur, *dit, *dps, *dfs;
  hc.in(&dB, B, b * nn);
  hc.in(&dC, C, b * nn);
  hc.in(&dT, T, b * nn);
  hc.in(&dR, R, b * n * k);
  hc.in(&de, eps, (eps_batched ? b : 1) * np * n_shock_steps * k);
  hc.in(&dx0, x0, (x0_batched ? b : 1) * (x0_paths ? np : 1) * n);
  hc.in(&dZ, Z, (z_batched ? b : 1) * p * n);
  hc.in(&dd, d, (d_batched ? b : 1) * p);
  hc.in(&dc, c_row, (c_batched ? b : 1) * n);
  hc.in(&dbound, bound, bound_batched ? b : 1);
  hc.io(&dS, status_io, b);
  hc.out(&dx, x_out, b * np * ns * n);
  hc.out(&dobs, obs_out, b * np * ns * p);
  hc.out(&dgap, gap_out, b * np * ns);
  hc.out(&dsh, shadow_out, b * np * ns);
  hc.out(&dplan, plan_out, b * np * ns * H);
  hc.out(&ddur, duration_out, b * np * ns);
  hc.out(&dit, iters_out, b * np * ns);
  hc.out(&dMz, Mz_out, b * H * H);
  hc.out(&dps, path_status_out, b * np);
  hc.out(&dfs, fail_step_out, b * np);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_constrained_simulate_batched(dB, dC, dT, dR, de, eps_batched, dx0, x0_batched, x0_paths, dZ, z_batched, dd, d_batched,
                                              dc, c_batched, dbound, bound_batched, shock, horizon, max_iter, dS, batch, n, k, p,
                                              n_paths, n_steps, n_shock_steps, rank_tol, dx, dobs, dgap, dsh, dplan, ddur, dit, dMz, dps,
                                              dfs, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_forecast_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                               const double* d, int d_batched, const double* Hdiag, int h_batched, const double* a0,
                               const double* P0, const int32_t* status, int batch, int m, int k, int p, int n_steps, double* a_out,
                               double* p_out, int full_cov, double* y_out, double* f_out) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, nullptr, p, 0, 0.0, 0.0};  // (no panel: the moments only)
  const ShockCov q{Q, q_mode};
  int rc = check_forecast(T, R, q, obs, a0, batch, m, k, n_steps, a_out, p_out, y_out, f_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0 || n_steps == 0) return DSGE_SUCCESS;
  ObsModel dobs;
  ShockCov dq;
  const double *dT, *dR, *da0, *dP0;
  const int32_t* dS;
  double *da, *dp, *dy, *df;
  const size_t mm = (size_t)batch * m * m, tm = (size_t)batch * n_steps * m;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, (size_t)batch * m * k);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.in(&da0, a0, (size_t)batch * m);
  hc.in(&dP0, P0, mm);
  hc.in(&dS, status, (size_t)batch);
  hc.out(&da, a_out, tm);
  hc.out(&dp, p_out, full_cov ? tm * m : tm);
  hc.out(&dy, y_out, (size_t)batch * n_steps * p);
  hc.out(&df, f_out, (size_t)batch * n_steps * p * p);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_forecast_batched(dT, dR, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched, dobs.Hdiag,
                                  dobs.h_batched, da0, dP0,
                                  dS, batch, m, k, p, n_steps, da, dp, full_cov, dy, df, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_policy_norms_batched_host(const double* A, const double* B, const double* C, const double* D, const double* T,
                                   const double* R, const int32_t* state_mask, int batch, int n, int k,
                                   double* det_norm_out, double* stoch_norm_out) {
  int rc = check_common(batch, n, 56);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!A || !B || !C || !D || !T || !R || !state_mask || !det_norm_out || !stoch_norm_out)
    return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  const double *dA, *dB, *dC, *dD, *dT, *dR;
  const int32_t* dM;
  double *d1, *d2;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, D, nk);
  hc.in(&dT, T, nn);
  hc.in(&dR, R, nk);
  hc.in(&dM, state_mask, n);
  hc.out(&d1, det_norm_out, batch);
  hc.out(&d2, stoch_norm_out, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_policy_norms_batched(dA, dB, dC, dD, dT, dR, dM, batch, n, k, d1, d2, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_backward_direct_batched_host(const double* A, const double* B, const double* D, int batch, int n, int k,
                                      double* T_out, double* R_out) {
  int rc = check_common(batch, n, DSGE_MAX_N_CR);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!A || !B || !D || !T_out || !R_out) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  const double *dA, *dB, *dD;
  double *dT, *dR;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dD, D, nk);
  hc.out(&dT, T_out, nn);
  hc.out(&dR, R_out, nk);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_backward_direct_batched(dA, dB, dD, batch, n, k, dT, dR, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_lyapunov_batched_host(const double* T, const double* R, const double* Q, int q_mode, int batch, int m, int k,
                               double* P0_out, double* RQR_out, int32_t* status) {
  int rc = check_common(batch, m, DSGE_MAX_N);
  if (rc) return rc;
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q_mode < 0 || q_mode > 3) return fail(DSGE_ERR_INVALID, "bad q_mode");
  if (!T || !R || !Q || !P0_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t mm = (size_t)batch * m * m, mk = (size_t)batch * m * k;
  ShockCov dq;
  const double *dT, *dR;
  double *dP, *dX;
  int32_t* dS;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, mk);
  hc.in(&dq, ShockCov{Q, q_mode}, batch, k);
  hc.out(&dP, P0_out, mm);
  hc.out(&dX, RQR_out, mm);
  hc.out(&dS, status, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_lyapunov_batched(dT, dR, dq.Q, dq.mode, batch, m, k, dP, dX, dS, hc.stream()))) return rc;
  return hc.finish();
}

int dsge_solve_kalman_logp_augmented_batched_host(const double* A, const double* B, const double* C, const double* D,
                                                  const double* Q, int q_mode, const double* Z, int z_batched,
                                                  const double* d, int d_batched, const double* Hdiag, int h_batched,
                                                  const double* y, int batch, int n, int k, int p, int T_len, int solver,
                                                  double tol, int max_iter, double jitter, double missing_fill, int m,
                                                  const int32_t* inv_var_order, int n_links, const int32_t* link_rows,
                                                  const int32_t* link_cols, int n_state_hint, int z_selector_hint,
                                                  int n_lead_hint, double* logp_out, int32_t* status_out,
                                                  double* T_aug_out, double* R_aug_out, double* resid_out) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_augmented(batch, n, k, obs, q, solver, m, n_links,
                           A && B && C && D && logp_out && status_out && (n_links == 0 || (link_rows && link_cols)));
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k, mm = (size_t)batch * m * m, mk = (size_t)batch * m * k;
  ObsModel dobs;
  ShockCov dq;
  const double *dA, *dB, *dC, *dD;
  const int32_t *dinv, *dlr, *dlc;
  double *dL, *dTa, *dRa, *dRes;
  int32_t* dS;
  hc.in(&dA, A, nn);
  hc.in(&dB, B, nn);
  hc.in(&dC, C, nn);
  hc.in(&dD, D, nk);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.in(&dinv, inv_var_order, n);
  hc.in(&dlr, link_rows, n_links);
  hc.in(&dlc, link_cols, n_links);
  hc.out(&dL, logp_out, batch);
  hc.out(&dS, status_out, batch);
  hc.out(&dTa, T_aug_out, mm);
  hc.out(&dRa, R_aug_out, mk);
  hc.out(&dRes, resid_out, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_solve_kalman_logp_augmented_batched(dA, dB, dC, dD, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched,
                                                     dobs.Hdiag, dobs.h_batched, dobs.y, batch, n, k, p, T_len, solver, tol, max_iter, jitter, missing_fill,
                                                     m, dinv, n_links, dlr, dlc, n_state_hint, z_selector_hint, n_lead_hint,
                                                     dL, dS, dTa, dRa, dRes, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_solve_kalman_logp_grad_batched_host(const double* A, const double* B, const double* C, const double* D,
                                             const double* q, int q_batched, const double* Z, int z_batched,
                                             const double* d, int d_batched, const double* Hdiag, int h_batched,
                                             const double* y, int batch, int n, int k, int p, int T_len, int solver,
                                             double tol, int max_iter, double jitter, double missing_fill,
                                             int n_filter_hint, int n_lead_hint, double* logp_out, int32_t* status_out,
                                             double* A_bar, double* B_bar, double* C_bar, double* D_bar, double* q_bar,
                                             double* d_bar, double* h_bar) {
  return grad_host(A, B, C, D, q, q_batched, Z, z_batched, d, d_batched, Hdiag, h_batched, y, batch, n, k, p, T_len, solver, tol,
                   max_iter, jitter, missing_fill, n_filter_hint, n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar,
                   q_bar, d_bar, h_bar, false, nullptr);
}

int dsge_solve_kalman_logp_grad_dense_z_batched_host(const double* A, const double* B, const double* C, const double* D,
                                                     const double* q, int q_batched, const double* Z, int z_batched,
                                                     const double* d, int d_batched, const double* Hdiag, int h_batched,
                                                     const double* y, int batch, int n, int k, int p, int T_len, int solver,
                                                     double tol, int max_iter, double jitter, double missing_fill,
                                                     int n_filter_hint, int n_lead_hint, double* logp_out,
                                                     int32_t* status_out, double* A_bar, double* B_bar, double* C_bar,
                                                     double* D_bar, double* q_bar, double* d_bar, double* h_bar,
                                                     double* Z_bar) {
  return grad_host(A, B, C, D, q, q_batched, Z, z_batched, d, d_batched, Hdiag, h_batched, y, batch, n, k, p, T_len, solver, tol,
                   max_iter, jitter, missing_fill, n_filter_hint, n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar,
                   q_bar, d_bar, h_bar, true, Z_bar);
}

int dsge_autocorrelation_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                      const double* Hdiag, int batch, int m, int k, int p, int n_lags, int lag_step,
                                      int correlation, double* acf_out, double* Sigma_out, int32_t* status) {
  int rc = check_common(batch, m, DSGE_MAX_N);
  if (rc) return rc;
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q_mode < 0 || q_mode > 3) return fail(DSGE_ERR_INVALID, "bad q_mode");
  if (n_lags < 0 || lag_step < 1) return fail(DSGE_ERR_INVALID, "n_lags >= 0 and lag_step >= 1 required");
  if (Z && (p < 1 || p > DSGE_MAX_P)) return fail(DSGE_ERR_INVALID, "p out of range (1..DSGE_MAX_P)");
  if (!T || !R || !Q || !acf_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const int dim = Z ? p : m;
  const size_t mm = (size_t)batch * m * m, mk = (size_t)batch * m * k;
  const size_t no = (size_t)batch * (n_lags + 1) * dim * dim;
  ShockCov dq;
  const double *dT, *dR, *dZ, *dH;
  double *dSig, *dO;
  int32_t* dS;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, mk);
  hc.in(&dq, ShockCov{Q, q_mode}, batch, k);
  hc.in(&dZ, Z, (size_t)p * m);
  hc.in(&dH, Hdiag, p);
  if (Sigma_out)  // (the device entry always writes the state covariance)
    hc.out(&dSig, Sigma_out, mm);
  else
    hc.space(&dSig, mm);
  hc.out(&dO, acf_out, no);
  hc.out(&dS, status, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_autocorrelation_batched(dT, dR, dq.Q, dq.mode, dZ, dH, batch, m, k, p, n_lags, lag_step, correlation, dO,
                                         dSig, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_kalman_logp_batched_host(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                  int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                  const double* y, int batch, int m, int k, int p, int T_len, double jitter,
                                  double missing_fill, int n_state_hint, int z_selector_hint, double* logp_out,
                                  int32_t* status_io) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman(batch, m, k, obs, q, T && R && logp_out && status_io);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t mm = (size_t)batch * m * m, mk = (size_t)batch * m * k;
  ObsModel dobs;
  ShockCov dq;
  const double *dT, *dR;
  double* dL;
  int32_t* dS;
  hc.in(&dT, T, mm);
  hc.in(&dR, R, mk);
  hc.in(&dq, q, batch, k);
  hc.in(&dobs, obs, batch, m);
  hc.io(&dS, status_io, batch);
  hc.out(&dL, logp_out, batch);
  if ((rc = hc.stage())) return rc;
  if ((rc = dsge_kalman_logp_batched(dT, dR, dq.Q, dq.mode, dobs.Z, dobs.z_batched, dobs.d, dobs.d_batched, dobs.Hdiag,
                                     dobs.h_batched, dobs.y, batch, m, k, p, T_len, jitter, missing_fill, n_state_hint, z_selector_hint, dL, dS, hc.stream())))
    return rc;
  return hc.finish();
}

int dsge_solve_kalman_logp_batched_host(const double* A, const double* B, const double* C, const double* D,
                                        const double* Q, int q_mode, const double* Z, int z_batched, const double* d,
                                        int d_batched, const double* Hdiag, int h_batched, const double* y, int batch,
                                        int n, int k, int p, int T_len, int solver, double tol, int max_iter,
                                        double jitter, double missing_fill, int n_state_hint, int z_selector_hint,
                                        int n_lead_hint, double* logp_out, int32_t* status_out, double* T_out,
                                        double* R_out, double* resid_out, int32_t* n_iter_out) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_pipeline(batch, n, k, obs, q, solver, A && B && C && D && logp_out && status_out);
  if (rc) return rc;
  HostCall hc;
  if ((rc = hc.begin())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  // Shared inputs first (stream 0, by stage()), then the batch in chunks on two streams: while the kernels of chunk c run,
  // the host stages chunk c+1 (pageable memory: hipMemcpyAsync returns once the runtime has staged the buffer), so
  // the PCIe transfer of the Jacobians overlaps the compute.  Outputs come back in one go at the end.
  // (per draw: space only, uploaded chunk by chunk below -- as are Q, Z, d, Hdiag when they are batched)
  ObsModel dobs;
  ShockCov dq;
  const double *dA, *dB, *dC, *dD;
  double *dL, *dT, *dR, *dRes;
  int32_t *dS, *dI;
  hc.space(&dA, nn);
  hc.space(&dB, nn);
  hc.space(&dC, nn);
  hc.space(&dD, nk);
  hc.in(&dq, q, batch, k, false);
  hc.in(&dobs, obs, batch, n, false);
  hc.out(&dL, logp_out, batch);
  hc.out(&dS, status_out, batch);
  hc.out(&dT, T_out, nn);
  hc.out(&dR, R_out, nk);
  hc.out(&dRes, resid_out, batch);
  hc.out(&dI, n_iter_out, batch);
  if ((rc = hc.stage())) return rc;
  HIP_TRY(hipStreamSynchronize(hc.stream(0)));
  const int n_chunks = (batch >= 2048) ? 4 : (batch >= 512 ? 2 : 1);
  const int per = (batch + n_chunks - 1) / n_chunks;
  for (int c = 0; c < n_chunks; ++c) {
    const int c0 = c * per;
    const int nb = (batch - c0 < per) ? batch - c0 : per;
    if (nb <= 0) break;
    hipStream_t st = hc.stream(c & 1);
    const size_t o2 = (size_t)c0 * n * n, ok = (size_t)c0 * n * k;
    const ObsModel ho = obs.at(c0, n), dc = dobs.at(c0, n);  // the chunk's slice, on the host and on the device
    const ShockCov hq = q.at(c0, k), dqc = dq.at(c0, k);
    auto up = [st](const double* dev, const double* host, size_t count) {  // a slice of a space-only buffer
      return hipMemcpyAsync(const_cast<double*>(dev), host, count * sizeof(double), hipMemcpyHostToDevice, st);
    };
    HIP_TRY(up(dA + o2, A + o2, (size_t)nb * n * n));
    HIP_TRY(up(dB + o2, B + o2, (size_t)nb * n * n));
    HIP_TRY(up(dC + o2, C + o2, (size_t)nb * n * n));
    HIP_TRY(up(dD + ok, D + ok, (size_t)nb * n * k));
    if (q.batched()) HIP_TRY(up(dqc.Q, hq.Q, q.elems(nb, k)));
    if (z_batched) HIP_TRY(up(dc.Z, ho.Z, (size_t)nb * p * n));
    if (d && d_batched) HIP_TRY(up(dc.d, ho.d, (size_t)nb * p));
    if (Hdiag && h_batched) HIP_TRY(up(dc.Hdiag, ho.Hdiag, (size_t)nb * p));
    // (pipeline_unchunked, not the public entry: that one would chunk again under dsge_options.pipeline_chunks)
    if ((rc = pipeline_unchunked(dA + o2, dB + o2, dC + o2, dD + ok, dqc, dc, nb, n, k, solver, tol, max_iter, n_state_hint,
                                 z_selector_hint, n_lead_hint, dL + c0, dS + c0, dT ? dT + o2 : nullptr, dR ? dR + ok : nullptr,
                                 dRes ? dRes + c0 : nullptr, dI ? dI + c0 : nullptr, st, 1, nullptr)))
      return rc;
  }
  for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamSynchronize(hc.stream(i)));
  return hc.finish();
}

}  // extern "C"
