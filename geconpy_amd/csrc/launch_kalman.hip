// Launcher of the Kalman log-likelihood kernels: executes the plan of dsge_kalman_plan.hpp (fast-path tile cascade + general kernel).
#include "dsge_host.hpp"
#include "dsge_kalman_launch.hpp"
#include "dsge_kalman_out.hpp"
#include "dsge_kalman_plan.hpp"
#include "dsge_kalman_tail.hpp"

namespace dsge_host {

long long* g_kalman_dbg = nullptr;  // debug: device buffer for per-phase cycles of draw 0
int32_t* g_kalman_steady_at = nullptr;
long long* g_kalman_timeline = nullptr;  // debug: device int64 [batch][8], see kalman_nt_kernel

namespace {
// The stream the two-wavefront head launch runs on, next to the caller's stream (fork / join by events): one per host thread and
// device, created on first use.  Two calls of one thread on two caller streams share it -- their heads then run one after the
// other, which is correct (events order them) and rare.
thread_local ThreadStream t_head;
// hand-off records of the fast kernel for kalman_tail_kernel: one buffer per (device, stream), grown on demand
StreamArenaPool g_tail_pool;

FilterArgs without_tail(FilterArgs a) {
  a.tail_rec = nullptr; a.tail_flag = nullptr; a.tail_from = nullptr;
  return a;
}

// the tail launches of the plan, over the whole batch's records, on stream ts
int launch_tails(const KalmanPlan& pl, const FilterArgs& a, hipStream_t ts) {
  const ObsModel& o = a.o;
  for (int i = 0; i < pl.n_tails; ++i) {
    const int m_lo = pl.tails[i].m_lo;
#define LAUNCH_TAIL4(MCV)                                                                                                      \
  hipLaunchKernelGGL((dsge::kalman_tail4_kernel<MCV>), dim3(a.batch), dim3(64), 0, ts, (const double*)a.tail_rec, a.tail_flag, \
                     o.y, a.batch, o.p, o.T_len, o.missing_fill, a.logp, a.status, a.steady_at, a.cv, m_lo)
    switch (pl.tails[i].mc) {
      case 0:
        hipLaunchKernelGGL(dsge::kalman_tail_kernel, dim3(a.batch), dim3(64), 0, ts, (const double*)a.tail_rec, a.tail_flag, o.y,
                           a.batch, o.p, o.T_len, o.missing_fill, a.logp, a.status, a.steady_at, a.cv);
        break;
      case 8: LAUNCH_TAIL4(8); break;
      case 16: LAUNCH_TAIL4(16); break;
      case 24: LAUNCH_TAIL4(24); break;
      default: LAUNCH_TAIL4(32); break;
    }
#undef LAUNCH_TAIL4
  }
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

// The NT kernel on one tile: a stamped instance under the hook (tools/kalman_phases.py), else head and bulk.
template <int BS, int SK>
int run_nt(const KalmanPlan& pl, const KalmanPlan::Valu& v, const FilterArgs& a, hipStream_t st) {
  if (v.family == KalmanFamily::nt_stamped) return launch_nt<BS, true, SK>(a.batch, st, v.lds, without_tail(a));
  if constexpr (BS <= 4) {
    if (v.family == KalmanFamily::nt2_stamped) return launch_nt2<BS, SK, true>(a.batch, st, v.lds, a);
  }
  // Head of the dispatch order on the two-wavefront kernel (dsge_kalman_nt2.hpp), on a second stream next to the bulk: the launch
  // ends with its slowest draws, and those run a full step in two thirds of the time there.
  // The HEAD runs on the caller's stream, where it starts the moment the solver ends; the BULK goes to the library's
  // second stream (fork / join by events).  The other way round the bulk, in stream order right behind the solver, fills
  // every CU's LDS before the cross-stream dependency of the head resolves, and the slow draws start LAST (measured).
  int rc;
  ThreadStream* hs = nullptr;
  hipStream_t bulk_st = st;
  ForkGuard head_guard{nullptr, st};  // (a return between fork and join still joins)
  if (v.head > 0 && v.head < a.batch) {
    hs = head_guard.side = &t_head;
    if ((rc = hs->fork(st))) return rc;
    bulk_st = hs->stream();
  }
  if constexpr (BS <= 4) {
    if (v.head > 0) {
      FilterArgs h = a;
      h.batch = v.head;
      if ((rc = launch_nt2<BS, SK>(v.head, st, v.lds_head, h))) return rc;
    }
  }
  if (v.head < a.batch) {
    FilterArgs b = a;
    b.batch = a.batch - v.head;
    b.dbg = g_kalman_timeline;
    if (b.order) b.order += v.head;
    if (!v.tail) b.tail_rec = nullptr;
    rc = v.tail ? launch_nt<BS, false, SK, true>(b.batch, bulk_st, v.lds, b) : launch_nt<BS, false, SK, false>(b.batch, bulk_st, v.lds, b);
    if (rc) return rc;
    if (hs && v.tail && (rc = launch_tails(pl, a, hs->stream()))) return rc;  // the bulk's tails next to the head, not behind it
  }
  // join: everything later on the caller's stream waits for the bulk (after an error: by the guard, which keeps it)
  return hs ? hs->join(st) : DSGE_SUCCESS;
}
}  // namespace

// dispatch key from the transition matrices themselves (any solver): see persistence_key_kernel
int launch_persistence_key(const double* T, const int32_t* status, int batch, int n, int32_t* key, hipStream_t st) {
  if (n > 64) return fail(DSGE_ERR_INVALID, "persistence key: n > 64");
  hipLaunchKernelGGL(dsge::persistence_key_kernel<64>, dim3(batch), dim3(64), 0, st, T, status, batch, n, key);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

bool kalman_folds_rqr(int m, int p, int k, int n_state_hint, int z_selector_hint) {
  const KalmanShape s{m, p, k, 0, 1, n_state_hint, z_selector_hint, true, false, false, false};  // (fold looks at none of the rest)
  return kalman_plan(s, opt(), g_kalman_dbg != nullptr).fold;
}

// p0_valid = 0: P0 is an uninitialised scratch buffer.  The fast kernels then compute the stationary
// covariance themselves (on the reduced model); only the draws that end up in the general kernel get
// their full-size P0 from the assemble kernel's Lyapunov pass (from RQR, which must be valid).
// Fast path (p <= 8): compact state block of at most s_cap columns; selector Z (gathers) or dense Z (one extra product per step).
// Draws that violate a hint come back flagged and are re-run by the next instance, at last by the general kernel.
int launch_kalman(const double* T, double* RQR, double* P0, int p0_valid, const ObsModel& o, int batch, int m, int n_state_hint,
                  int z_selector_hint, double* logp, int32_t* status, hipStream_t st, const int32_t* order_key, const double* Rsel,
                  const ShockCov& q, int k_shocks, const unsigned long long* colmask, int rerun_all) {
  const KalmanShape shape{m, o.p, k_shocks, o.T_len, batch, n_state_hint, z_selector_hint, Rsel && q.Q, order_key != nullptr,
                          p0_valid != 0, rerun_all != 0};
  const KalmanPlan pl = kalman_plan(shape, opt(), g_kalman_dbg != nullptr);
  if (Rsel && !pl.fold) return fail(DSGE_ERR_INVALID, "launch_kalman: R given but the filter kernel cannot form R Q R' itself");
  int rc;
  FilterArgs a;
  a.T = T; a.RQR = RQR; a.P0 = p0_valid ? P0 : nullptr; a.o = o; a.batch = batch; a.m = m;
  a.cv = filter_conv(o.jitter);  // the call's jitter + the conventions of dsge_options
  a.steady_tol = opt().kalman_steady_tol; a.logp = logp; a.status = status; a.steady_at = g_kalman_steady_at;
  if (pl.tiny_u) {
    const unsigned blocks = (batch + 63) / 64;
    if ((rc = pl.tiny_u == 4 ? launch_tiny<4, 3>(blocks, st, a) : launch_tiny<6, 3>(blocks, st, a))) return rc;
  }
  if (pl.reserve_bytes) {
    void* base = nullptr;
    if ((rc = g_tail_pool.reserve(pl.reserve_bytes, st, &base))) return rc;
    int32_t* ints = (int32_t*)base;  // [batch] flags, [1] scan result, [batch] dispatch order
    if (pl.want_tail) {  // records, flags and the index from which the missing-data mask of the shared panel y no longer changes
      a.tail_flag = ints;
      a.tail_from = ints + batch;
      a.tail_rec = (double*)((char*)base + pl.int_bytes);
      HIP_TRY(hipMemsetAsync(ints, 0, ((size_t)batch + 1) * sizeof(int32_t), st));
      hipLaunchKernelGGL(dsge::kalman_mask_scan_kernel, dim3(1), dim3(64), 0, st, o.y, o.p, o.T_len, o.missing_fill, ints + batch);
    }
    if (pl.want_order) {
      a.order = ints + batch + 1;
      hipLaunchKernelGGL(dsge::kalman_order_kernel<1024>, dim3(1), dim3(1024), 0, st, order_key, batch, ints + batch + 1);
    }
    HIP_TRY(hipGetLastError());
  }
  FilterArgs f = a;  // the fast kernels'
  f.dbg = g_kalman_dbg; f.Rsel = pl.fold ? Rsel : nullptr; f.q = q; f.k_shocks = k_shocks; f.colmask = colmask;
  for (int i = 0; i < pl.n_mf; ++i) {
    if ((rc = launch_kalman_mf(pl.mf[i], f, st))) return rc;
  }
  for (int i = 0; i < pl.n_valu; ++i) {
    const KalmanPlan::Valu& v = pl.valu[i];
    f.s_cap = v.s_cap; f.rerun = v.rerun;
    const unsigned grid = v.rerun ? rerun_grid(batch) : batch;  // (of the kalman_sel_kernel instances)
    rc = DSGE_ERR_INVALID;  // (too_wide: no instance)
    DISPATCH_BS(v.bs, 8, {
      switch (v.family) {
        case KalmanFamily::sel_mfma16:
          if constexpr (BS == 2 || BS == 3) rc = launch_sel<BS, true, true>(grid, st, v.lds, without_tail(f));
          break;
        case KalmanFamily::sel_tail: rc = launch_sel<BS, true, false, true>(grid, st, v.lds, f); break;
        case KalmanFamily::sel: rc = launch_sel<BS, true>(grid, st, v.lds, without_tail(f)); break;
        case KalmanFamily::sel_dense: rc = launch_sel<BS, false>(grid, st, v.lds, without_tail(f)); break;
        case KalmanFamily::no_fit: rc = DSGE_SUCCESS; break;  // the general kernel handles everything
        case KalmanFamily::too_wide: break;
        default: rc = v.sk < 8 * BS ? run_nt<BS, (BS == 4 ? 20 : 8 * BS)>(pl, v, f, st) : run_nt<BS, 8 * BS>(pl, v, f, st); break;
      }
    });
    if (rc) return rc;
  }
  if (pl.n_tails && (rc = launch_tails(pl, a, st))) return rc;
  if (pl.fold) {  // the general kernel's inputs for the draws the fast kernel handed on: their sym(R Q R') after all
    if ((rc = launch_rqr(Rsel, q.Q, q.batched(), batch, m, k_shocks, status, RQR, st, 1))) return rc;
  }
  // full-size P0 for the general kernel: flagged draws only when a fast kernel ran, else every draw
  if (pl.p0_pass && (rc = assemble_p0_from_rqr(T, RQR, batch, m, P0, status, pl.p0_pass == 2, st))) return rc;
  a.P0 = P0; a.rerun = pl.general_rerun;
  rc = DSGE_ERR_INVALID;
  DISPATCH_BS(pl.general_bs, 8,
              rc = launch_general<BS>(pl.general_rerun ? rerun_grid(batch) : batch, st, dsge::KfSmem<BS>::bytes(o.p), a));
  return rc;
}

// per-step filter outputs (dsge_kalman_out.hpp)
int launch_kalman_outputs(const double* T, const double* RQR, const double* P0, const ObsModel& o, int batch, int m, double* ll,
                          double* a_pred, double* a_filt, double* p_pred, double* p_filt, int full_cov, int32_t* status,
                          hipStream_t st) {
  dsge::KoArgs a{};
  a.T = T; a.RQR = RQR; a.P0 = P0; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.ll = ll; a.a_pred = a_pred; a.a_filt = a_filt;
  a.p_pred = p_pred; a.p_filt = p_filt; a.status = status; a.batch = batch; a.m = m; a.p = o.p; a.T_len = o.T_len;
  a.z_batched = o.z_batched; a.d_batched = o.d_batched; a.h_batched = o.h_batched; a.full_cov = full_cov; a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  const size_t lds = dsge::ko_lds_doubles(m, o.p) * sizeof(double);
  int rc;
  if ((rc = set_lds(dsge::kalman_outputs_kernel, lds))) return rc;
  hipLaunchKernelGGL(dsge::kalman_outputs_kernel, dim3(batch), dim3(dsge::KO_THREADS), lds, st, a);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
