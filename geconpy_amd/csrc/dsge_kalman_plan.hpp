// The dispatch of the Kalman log-likelihood kernels as data.  kalman_plan() is a pure function of the shape, the options and the
// phase-stamp hook: no HIP call, no global, no heap.  launch_kalman executes the plan, kalman_folds_rqr reports its `fold`, so the
// rule exists once.  The plan lists, in launch order: the tiny kernel, the scratch of tail hand-off and dispatch order, the
// tile-layout instances, the VALU tiles, the tail launches, the general kernel's inputs and the general kernel.
#pragma once
#include "dsge_host.hpp"
#include "dsge_kalman2.hpp"
#include "dsge_kalman_mf.hpp"
#include "dsge_kalman_nt.hpp"
#include "dsge_kalman_nt2.hpp"
#include "dsge_kernels.hpp"

namespace dsge_host {

struct KalmanShape {
  int m, p, k_shocks, T_len, batch, n_state_hint, z_selector_hint;
  bool r_given;    // the selection matrix and a diagonal Q came with the call
  bool order_key;  // a dispatch key came with the call
  bool p0_valid;
  bool rerun_all;  // every launch is a second pass on the flagged draws
};

enum class KalmanFamily {
  sel_mfma16,   // kalman_sel_kernel<BS, true, true>: products on the 16 x 16 x 4 matrix instruction (BS 2, 3)
  sel_tail,     // kalman_sel_kernel<BS, true, false, true>: hands steady tails on; takes no Rsel
  nt,           // kalman_nt_kernel<BS, false, SK, tail>, its head on kalman_nt2_kernel<BS, SK>
  nt_stamped,   // kalman_nt_kernel<BS, true, SK>
  nt2_stamped,  // kalman_nt2_kernel<BS, SK, true>
  sel,          // kalman_sel_kernel<BS, true>
  sel_dense,    // kalman_sel_kernel<BS, false>: dense Z
  no_fit,       // dense Z beyond the LDS: nothing launched, the general kernel takes every draw
  too_wide      // a tile beyond 64 variables: the call is refused here
};

struct KalmanPlan {
  int tiny_u = 0;  // kalman_tiny_kernel<tiny_u, 3> on every draw first (4 or 6); 0: not run
  // scratch in front of the fast kernels: [batch] tail flags, [1] mask scan, [batch] dispatch order in int_bytes, then the records
  bool want_tail = false, want_order = false;
  size_t int_bytes = 0, reserve_bytes = 0;
  struct Mf {  // kalman_mf_kernel<kt, tm, stamped>, full grid
    int kt, tm, wt;  // wt: doubles of its W' buffer, which stages R
    bool stamped, rerun;
    size_t lds;
  } mf[2];
  int n_mf = 0;
  bool mf_covers = false;  // the tile-layout instances take everything the VALU tiles could: those are skipped
  struct Valu {
    KalmanFamily family;
    int bs, sk, s_cap;
    bool tail, rerun;
    int head;                // nt: draws at the head of the order on kalman_nt2_kernel (caller's stream); the bulk forks when 0 < head < batch
    size_t lds, lds_head;
    int stage;               // doubles of the buffer that stages R (nt, nt2 and their stamped instances; else 0)
  } valu[2];
  int n_valu = 0;
  struct Tail {  // kalman_tail4_kernel<mc> on the draws with m_lo < m <= mc; mc = 0: the two-step kalman_tail_kernel
    int mc, m_lo;
  } tails[4];
  int n_tails = 0;
  bool fold = false;         // the fast kernels form sym(R Q R') themselves; launch_rqr then runs for the flagged draws only
  int p0_pass = 0;           // assemble_p0_from_rqr: 0 not run (P0 valid), 1 every draw, 2 flagged draws only
  int general_bs = 0;        // kalman_kernel<general_bs>; beyond 8 the call is refused
  bool general_rerun = false;  // second pass on rerun_grid, else every draw on the full grid
};

namespace plan_detail {
template <int KT, int TM>
inline void mf_sizes(KalmanPlan::Mf& f) {
  f.wt = dsge::KmfSmem<KT, TM>::WT;
  f.lds = dsge::KmfSmem<KT, TM>::bytes;
}
inline void mf_instance(KalmanPlan::Mf& f) {
  switch (10 * f.kt + f.tm) {
    case 33: return mf_sizes<3, 3>(f);
    case 35: return mf_sizes<3, 5>(f);
    case 44: return mf_sizes<4, 4>(f);
    case 46: return mf_sizes<4, 6>(f);
    case 55: return mf_sizes<5, 5>(f);
    default: return mf_sizes<5, 7>(f);
  }
}

// One VALU tile.  The instances are tried smallest first: each flags the draws that do not fit it, the next picks up those.
template <int BS>
void valu_tile(KalmanPlan::Valu& v, const KalmanShape& s, const Options& opt, bool dbg, const KalmanPlan& pl, size_t r_doubles) {
  constexpr int NP = 8 * BS;
  constexpr int SK_NARROW = (BS == 4) ? 20 : NP;  // (the 32-wide tile only: on the 24-wide one the 20-column instance measured slower)
  const int hint = s.n_state_hint;
  v.s_cap = (hint > 0 && hint < NP) ? ((hint + BS - 1) / BS) * BS : NP;
  if (v.s_cap > NP) v.s_cap = NP;
  if (!s.z_selector_hint) {  // dense Z: one extra product per step, no reduction assumed
    v.lds = dsge::Kf2Smem<BS>::bytes(v.s_cap, true);
    v.family = v.lds > LDS_LIMIT ? KalmanFamily::no_fit : KalmanFamily::sel_dense;
    return;
  }
  v.lds = dsge::Kf2Smem<BS>::bytes(v.s_cap, false);
  if ((BS == 2 || BS == 3) && opt.kalman_mfma == 1) {
    v.family = KalmanFamily::sel_mfma16;
  } else if (pl.want_tail && BS <= 4 && (!opt.kalman_nt_products || dbg)) {
    v.family = KalmanFamily::sel_tail;
  } else if (opt.kalman_nt_products) {
    // SK = 20 (up to 20 state variables: the 32-wide tile at 20 KB of LDS) or the generic SK = NP.  With R folded in, the kernel
    // stages the m x k selection matrix in its W' buffer, which is narrower too.
    const bool stage_fits = !pl.fold || r_doubles <= (size_t)NP * (SK_NARROW + 2);
    const bool narrow = SK_NARROW < NP && v.s_cap <= SK_NARROW && opt.kalman_narrow && stage_fits;
    v.sk = narrow ? SK_NARROW : NP;
    v.stage = NP * (v.sk + 2);
    v.tail = pl.want_tail && !dbg && BS <= 4;  // (the record holds a tile of at most 32 variables)
    const size_t lds2 = narrow ? dsge::Knt2Smem<BS, SK_NARROW>::bytes(v.s_cap) : dsge::Knt2Smem<BS, NP>::bytes(v.s_cap);
    v.lds = narrow ? dsge::KntSmem<BS, SK_NARROW>::bytes(v.s_cap) : dsge::KntSmem<BS, NP>::bytes(v.s_cap);
    if (dbg && BS <= 4 && opt.kalman_head_draws != 0) {
      v.family = KalmanFamily::nt2_stamped;
      v.lds = lds2;
    } else if (dbg) {
      v.family = KalmanFamily::nt_stamped;
    } else {
      v.family = KalmanFamily::nt;
      int head = (BS <= 4 && !v.rerun) ? opt.kalman_head_draws : 0;
      if (head < 0 || head > s.batch) head = s.batch;
      if (head > 0 && head < s.batch && !pl.want_order) head = 0;  // (without an order the first indices are no slower than the rest)
      if (head > 0 && lds2 > LDS_LIMIT) head = 0;
      v.head = head;
      v.lds_head = head > 0 ? lds2 : 0;
    }
  } else {
    v.family = KalmanFamily::sel;
  }
}
}  // namespace plan_detail

inline KalmanPlan kalman_plan(const KalmanShape& s, const Options& opt, bool dbg) {
  KalmanPlan pl{};
  const int hint = s.n_state_hint, m = s.m, p = s.p, k = s.k_shocks;
  const bool fast = p <= 8, sel = s.z_selector_hint != 0;
  const bool reduced = sel && hint > 0 && hint < m;  // the fast kernels filter states + observed non-states only
  const size_t r_doubles = (size_t)m * ((k + 1) & ~1);
  bool launched = s.rerun_all;  // a fast kernel ran: what follows is a second pass

  // Small models (reduced filter of at most 6 variables, p <= 3, selector Z): one thread per draw, all in registers.
  const bool tiny_shape = opt.kalman_tiny && sel && p <= 3 && hint > 0 && hint + p <= 6;
  if (tiny_shape && !s.rerun_all) {
    pl.tiny_u = hint + p <= 4 ? 4 : 6;
    launched = true;
  }
  // fold: the NT kernel or a tile-layout instance takes every draw first (no tiny kernel, no 16 x 16 x 4 variant and no
  // kalman_sel_kernel tail instance in front of them -- that one runs under kalman_block when the NT kernel is off or the hook is
  // armed), and R fits the staging area of the smallest tile tried, its NP x (NP + 2) W' buffer.
  const int lo = tile_bs(reduced ? hint : m);
  pl.fold = s.r_given && fast && sel && opt.kalman_nt_products && opt.kalman_mfma != 1 && k >= 1 && k <= dsge::RQR_KMAX &&
            !tiny_shape && !(opt.kalman_block && dbg) && lo <= 8 && r_doubles <= (size_t)(8 * lo) * (8 * lo + 2);

  // Tail hand-off (selector Z: the kernels decide per draw) and dispatch order
  pl.want_tail = fast && sel && opt.kalman_block && s.T_len >= 8;
  pl.want_order = fast && s.order_key && opt.kalman_order && s.batch >= 512;
  if (pl.want_tail || pl.want_order) {
    pl.int_bytes = ((2 * (size_t)s.batch + 1) * sizeof(int32_t) + 255) & ~(size_t)255;
    pl.reserve_bytes = pl.int_bytes + (pl.want_tail ? (size_t)s.batch * dsge::KT_REC * sizeof(double) : 0);
  }

  // The covariance in the tile layout of the 4 x 4 x 4 matrix instruction: KT tiles hold the state block (9 .. 20 variables), TM =
  // KT tiles the retained variables and, when observed non-states may add to them, TM = KT + 2 as a second pass.  An instance whose
  // W' buffer cannot stage R is skipped.  Under the hook only the stamped instance of the SW-shaped size exists.
  if (fast && sel && opt.kalman_mfma == 2 && opt.kalman_nt_products && !pl.want_tail && opt.kalman_head_draws == 0 && hint >= 9 &&
      hint <= 20) {
    const int kt = (hint + 3) / 4;
    const bool wide = hint + p > 4 * kt && hint < m;
    const int n_wanted = dbg ? (kt == 5 ? 1 : 0) : (wide ? 2 : 1);
    for (int i = 0; i < n_wanted; ++i) {
      KalmanPlan::Mf f{kt, kt + 2 * i, 0, dbg, launched || pl.n_mf > 0, 0};
      plan_detail::mf_instance(f);
      if (!pl.fold || r_doubles <= (size_t)f.wt) pl.mf[pl.n_mf++] = f;
    }
    pl.mf_covers = !dbg && pl.n_mf == n_wanted;
    launched = launched || pl.n_mf > 0;
  }

  // The VALU tiles.  The reduced dimension u is only known per draw on the device (hint <= u <= hint + p for a selector), so the
  // tile of the hint comes first and the tile of hint + p second.
  if (fast && !pl.mf_covers) {
    int tiles[2] = {tile_bs(reduced ? hint : m), 0};
    pl.n_valu = 1;
    if (reduced) {
      tiles[1] = tile_bs(hint + p < m ? hint + p : m);
      if (tiles[1] != tiles[0]) pl.n_valu = 2;
    }
    for (int it = 0; it < pl.n_valu; ++it) {
      KalmanPlan::Valu& v = pl.valu[it];
      v = KalmanPlan::Valu{KalmanFamily::too_wide, tiles[it], 0, 0, false, launched, 0, 0, 0, 0};
      DISPATCH_BS(v.bs, 8, plan_detail::valu_tile<BS>(v, s, opt, dbg, pl, r_doubles));
      if (v.family == KalmanFamily::too_wide) {
        pl.n_valu = it + 1;
        return pl;
      }
      launched = launched || v.family != KalmanFamily::no_fit;
    }
  }

  // The tails: four steps per trip, one launch per tile width that can have written records -- the instance MC takes the draws with
  // m_lo < m <= MC, the narrowest also the smaller ones.  kalman_block = 2: the two-step kernel of round 2 (kept for comparison).
  if (pl.want_tail && opt.kalman_block == 2) {
    pl.tails[pl.n_tails++] = {0, 0};
  } else if (pl.want_tail) {
    const int bs_lo = tile_bs(reduced ? hint : m), bs_hi = tile_bs(sel && hint > 0 && hint + p < m ? hint + p : m);
    for (int b = bs_lo; b <= bs_hi && b <= 4; ++b) pl.tails[pl.n_tails++] = {8 * b, b == bs_lo ? 0 : 8 * (b - 1)};
  }

  pl.p0_pass = s.p0_valid ? 0 : (launched ? 2 : 1);
  pl.general_bs = tile_bs(m);
  pl.general_rerun = launched;
  return pl;
}

// launch_kalman_mf.hip: one tile-layout instance of the plan, with launch_kalman's arguments (dsge_kalman_launch.hpp)
struct FilterArgs;
int launch_kalman_mf(const KalmanPlan::Mf& f, FilterArgs a, hipStream_t st);

}  // namespace dsge_host
