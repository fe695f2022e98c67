// Stand-alone check of kalman_plan() (csrc/dsge_kalman_plan.hpp) on the host: the instance lists of named shapes and the plan's
// properties over a sweep of shapes, hints and options.  No HIP call; built host-only by tests/test_kalman_plan.py.
#include <cstdio>
#include <initializer_list>

#include "dsge_kalman_plan.hpp"
#include "dsge_kalman_tiny.hpp"

using namespace dsge_host;
using F = KalmanFamily;

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(...)                                                             \
  do {                                                                         \
    if (!(__VA_ARGS__)) {                                                            \
      if (++g_failed <= 40) std::printf("FAILED [%s] line %d: %s\n", g_case, __LINE__, #__VA_ARGS__); \
    }                                                                          \
  } while (0)

// the SW-shaped fused call: 40 variables, 18 states, 7 observables (selector), 7 shocks, 4096 draws, R given, an order key
static KalmanShape sw() { return KalmanShape{40, 7, 7, 200, 4096, 18, 1, true, true, false, false}; }

static bool is_mf(const KalmanPlan::Mf& f, int kt, int tm, bool stamped, bool rerun) {
  return f.kt == kt && f.tm == tm && f.stamped == stamped && f.rerun == rerun;
}
static bool is_valu(const KalmanPlan::Valu& v, F family, int bs, bool rerun) { return v.family == family && v.bs == bs && v.rerun == rerun; }

static void named_shapes() {
  const Options def;
  {
    g_case = "SW-shaped, defaults";
    const KalmanPlan pl = kalman_plan(sw(), def, false);
    CHECK(pl.tiny_u == 0 && pl.n_mf == 2 && is_mf(pl.mf[0], 5, 5, false, false) && is_mf(pl.mf[1], 5, 7, false, true));
    CHECK(pl.mf[0].lds == dsge::KmfSmem<5, 5>::bytes && pl.mf[1].lds == dsge::KmfSmem<5, 7>::bytes && pl.mf[0].wt == 440);
    CHECK(pl.mf_covers && pl.n_valu == 0 && pl.n_tails == 0);
    CHECK(pl.general_bs == 5 && pl.general_rerun && pl.p0_pass == 2);
    CHECK(pl.fold && pl.want_order && !pl.want_tail);
    CHECK(pl.int_bytes == 32768 + 256 && pl.reserve_bytes == pl.int_bytes);  // 2 * 4096 + 1 ints, rounded up to 256 bytes
  }
  {
    g_case = "kalman_mfma = 0";
    Options o;
    o.kalman_mfma = 0;
    const KalmanPlan pl = kalman_plan(sw(), o, false);
    CHECK(pl.n_mf == 0 && !pl.mf_covers && pl.n_valu == 2 && pl.fold);
    CHECK(is_valu(pl.valu[0], F::nt, 3, false) && pl.valu[0].sk == 24 && pl.valu[0].s_cap == 18 && !pl.valu[0].tail && pl.valu[0].head == 0);
    CHECK(pl.valu[0].lds == dsge::KntSmem<3, 24>::bytes(18));
    CHECK(is_valu(pl.valu[1], F::nt, 4, true) && pl.valu[1].sk == 20 && pl.valu[1].s_cap == 20 && !pl.valu[1].tail && pl.valu[1].head == 0);
    CHECK(pl.valu[1].lds == dsge::KntSmem<4, 20>::bytes(20));
    CHECK(pl.general_bs == 5 && pl.general_rerun);
  }
  for (int block = 0; block <= 1; ++block) {
    g_case = block ? "kalman_nt_products = 0, kalman_block = 1" : "kalman_nt_products = 0";
    Options o;
    o.kalman_nt_products = 0;
    o.kalman_block = block;
    KalmanShape s = sw();
    s.r_given = false;  // (the caller asked kalman_folds_rqr first)
    const KalmanPlan pl = kalman_plan(s, o, false);
    const F fam = block ? F::sel_tail : F::sel;
    CHECK(pl.n_mf == 0 && pl.n_valu == 2 && is_valu(pl.valu[0], fam, 3, false) && is_valu(pl.valu[1], fam, 4, true));
    CHECK(pl.valu[0].lds == dsge::Kf2Smem<3>::bytes(18) && pl.valu[1].lds == dsge::Kf2Smem<4>::bytes(20));
    s.r_given = true;
    CHECK(!kalman_plan(s, o, false).fold && !pl.fold);
    CHECK(pl.want_tail == (block != 0) && pl.n_tails == (block ? 2 : 0));
    if (block) {
      CHECK(pl.tails[0].mc == 24 && pl.tails[0].m_lo == 0 && pl.tails[1].mc == 32 && pl.tails[1].m_lo == 24);
      CHECK(pl.reserve_bytes == pl.int_bytes + (size_t)4096 * dsge::KT_REC * sizeof(double));
    }
  }
  {
    g_case = "kalman_head_draws = -1";
    Options o;
    o.kalman_head_draws = -1;
    const KalmanPlan pl = kalman_plan(sw(), o, false);
    CHECK(pl.n_mf == 0 && pl.n_valu == 2 && is_valu(pl.valu[0], F::nt, 3, false) && pl.valu[0].head == 4096);  // nt2, no bulk
    CHECK(pl.valu[0].lds_head == dsge::Knt2Smem<3, 24>::bytes(18));
    CHECK(is_valu(pl.valu[1], F::nt, 4, true) && pl.valu[1].head == 0);  // a second pass has no head
  }
  {
    g_case = "kalman_head_draws = 128, with and without an order";
    Options o;
    o.kalman_head_draws = 128;
    KalmanPlan pl = kalman_plan(sw(), o, false);
    CHECK(pl.want_order && pl.n_valu == 2 && is_valu(pl.valu[0], F::nt, 3, false) && pl.valu[0].head == 128);  // bulk: 4096 - 128 forked
    CHECK(pl.valu[1].head == 0);
    KalmanShape s = sw();
    s.order_key = false;
    pl = kalman_plan(s, o, false);
    CHECK(!pl.want_order && pl.valu[0].head == 0);
  }
  {
    g_case = "no hints";
    KalmanShape s = sw();
    s.n_state_hint = 0;
    s.z_selector_hint = 0;
    s.r_given = false;
    const KalmanPlan pl = kalman_plan(s, def, false);
    CHECK(pl.n_mf == 0 && pl.n_valu == 1 && is_valu(pl.valu[0], F::sel_dense, 5, false) && pl.valu[0].s_cap == 40);
    CHECK(pl.valu[0].lds == dsge::Kf2Smem<5>::bytes(40, true) && !pl.fold && pl.general_rerun);
  }
  {
    g_case = "p = 9";
    KalmanShape s = sw();
    s.p = 9;
    const KalmanPlan pl = kalman_plan(s, def, false);
    CHECK(pl.tiny_u == 0 && pl.n_mf == 0 && pl.n_valu == 0 && pl.n_tails == 0 && !pl.fold && !pl.want_order && pl.reserve_bytes == 0);
    CHECK(pl.general_bs == 5 && !pl.general_rerun && pl.p0_pass == 1);
  }
  for (int hint = 1; hint <= 5; ++hint) {
    g_case = "tiny";
    KalmanShape s = sw();
    s.m = 12;
    s.p = 1;
    s.n_state_hint = hint;
    const KalmanPlan pl = kalman_plan(s, def, false);
    CHECK(pl.tiny_u == (hint + 1 <= 4 ? 4 : 6) && !pl.fold && pl.n_valu >= 1 && pl.valu[0].rerun && pl.general_rerun);
  }
  for (int hint : {12, 16}) {
    g_case = "hint 12 / 16";
    KalmanShape s = sw();
    s.n_state_hint = hint;
    const KalmanPlan pl = kalman_plan(s, def, false);
    const int kt = hint / 4;
    CHECK(pl.n_mf == 2 && is_mf(pl.mf[0], kt, kt, false, false) && is_mf(pl.mf[1], kt, kt + 2, false, true) && pl.mf_covers);
    CHECK(!pl.fold);  // 40 x 8 doubles of R are beyond the 16 x 18 staging area of the 16-wide tile
    s.m = 30;
    const KalmanPlan small = kalman_plan(s, def, false);  // 30 x 8 fit there, but not the 12 x 14 W' buffer of <3, 3>
    CHECK(small.fold && small.n_mf == (hint == 16 ? 2 : 1) && small.mf[small.n_mf - 1].tm == kt + 2 && small.mf_covers == (hint == 16));
  }
  {
    g_case = "k = 11";
    KalmanShape s = sw();
    s.k_shocks = 11;
    const KalmanPlan pl = kalman_plan(s, def, false);
    static_assert(dsge::KmfSmem<5, 5>::WT == 440 && 40 * 12 > 440, "the staged R of 11 shocks is beyond the <5, 5> instance");
    CHECK(pl.fold && pl.n_mf == 1 && is_mf(pl.mf[0], 5, 7, false, false) && !pl.mf_covers);
    CHECK(pl.n_valu == 2 && is_valu(pl.valu[0], F::nt, 3, true) && is_valu(pl.valu[1], F::nt, 4, true));
  }
  {
    g_case = "k = 17";
    KalmanShape s = sw();
    s.k_shocks = 17;
    CHECK(!kalman_plan(s, def, false).fold);
    s.k_shocks = 16;
    s.m = 24;
    s.n_state_hint = 0;
    CHECK(kalman_plan(s, def, false).fold);
  }
  {
    g_case = "hook armed";
    KalmanPlan pl = kalman_plan(sw(), def, true);
    CHECK(pl.n_mf == 1 && is_mf(pl.mf[0], 5, 5, true, false) && !pl.mf_covers && pl.fold);
    CHECK(pl.n_valu == 2 && is_valu(pl.valu[0], F::nt_stamped, 3, true) && is_valu(pl.valu[1], F::nt_stamped, 4, true));
    Options o;
    o.kalman_head_draws = -1;
    pl = kalman_plan(sw(), o, true);
    CHECK(pl.n_mf == 0 && is_valu(pl.valu[0], F::nt2_stamped, 3, false) && pl.valu[0].lds == dsge::Knt2Smem<3, 24>::bytes(18));
    // the two copies of the rule the plan replaces disagreed here: kalman_sel_kernel's tail instance runs and takes no Rsel
    o = Options();
    o.kalman_block = 1;
    pl = kalman_plan(sw(), o, true);
    CHECK(!pl.fold && is_valu(pl.valu[0], F::sel_tail, 3, false) && is_valu(pl.valu[1], F::sel_tail, 4, true));
  }
  {
    g_case = "rerun_all";
    KalmanShape s = sw();
    s.rerun_all = true;
    KalmanPlan pl = kalman_plan(s, def, false);
    CHECK(pl.n_mf == 2 && pl.mf[0].rerun && pl.mf[1].rerun && pl.general_rerun && pl.p0_pass == 2);
    s.m = 12;
    s.p = 1;
    s.n_state_hint = 3;
    pl = kalman_plan(s, def, false);
    CHECK(pl.tiny_u == 0 && pl.n_valu == 1 && pl.valu[0].rerun && pl.general_rerun);
  }
}

static long sweep() {
  long n = 0;
  const int ms[] = {1, 3, 8, 9, 17, 24, 25, 33, 40, 64};
  const int hints[] = {0, 1, 3, 5, 9, 12, 16, 18, 20, 21, 31, 64};
  const struct { int batch, T_len; bool order; } calls[] = {{1, 7, false}, {511, 8, true}, {512, 8, true}, {4096, 7, true}, {4096, 8, false}};
  g_case = "sweep";
  for (int tiny = 0; tiny <= 1; ++tiny)
  for (int block = 0; block <= 2; ++block)
  for (int mfma = 0; mfma <= 2; ++mfma)
  for (int ntp = 0; ntp <= 1; ++ntp)
  for (int narrow = 0; narrow <= 1; ++narrow)
  for (int head : {0, -1, 128})
  for (int order = 0; order <= 1; ++order) {
    Options o;
    o.kalman_tiny = tiny; o.kalman_block = block; o.kalman_mfma = mfma; o.kalman_nt_products = ntp; o.kalman_narrow = narrow;
    o.kalman_head_draws = head; o.kalman_order = order;
    for (int m : ms)
    for (int p : {1, 3, 4, 7, 8, 9})
    for (int k : {0, 1, 7, 10, 11, 16, 17})
    for (int hint : hints)
    for (int zsel = 0; zsel <= 1; ++zsel)
    for (const auto& c : calls)
    for (int flags = 0; flags < 4; ++flags) {
      const bool rerun_all = flags & 1, dbg = flags & 2;
      if (p > m) continue;
      const KalmanShape s{m, p, k, c.T_len, c.batch, hint, zsel, k > 0, c.order, c.batch == 1, rerun_all};
      const KalmanPlan pl = kalman_plan(s, o, dbg);
      ++n;
      const size_t r_doubles = (size_t)m * ((k + 1) & ~1);
      // 1. fold: every fast instance takes Rsel and can stage it
      if (pl.fold) {
        CHECK(pl.tiny_u == 0 && s.r_given);
        for (int i = 0; i < pl.n_mf; ++i) CHECK((size_t)pl.mf[i].wt >= r_doubles);
        for (int i = 0; i < pl.n_valu; ++i) {
          const KalmanPlan::Valu& v = pl.valu[i];
          CHECK(v.family == F::nt || v.family == F::nt_stamped || v.family == F::nt2_stamped);
          CHECK((size_t)v.stage >= r_doubles);
        }
        CHECK(pl.n_mf + pl.n_valu > 0);
      }
      // 2. LDS
      for (int i = 0; i < pl.n_mf; ++i) CHECK(pl.mf[i].lds <= LDS_LIMIT);
      for (int i = 0; i < pl.n_valu; ++i)
        CHECK(pl.valu[i].family == F::no_fit || (pl.valu[i].lds <= LDS_LIMIT && pl.valu[i].lds_head <= LDS_LIMIT));
      // 3. the first fast launch takes every draw unless rerun_all, every later one the flagged draws
      int n_fast = 0;
      if (pl.tiny_u) {
        CHECK(!rerun_all);
        ++n_fast;
      }
      for (int i = 0; i < pl.n_mf; ++i) CHECK(pl.mf[i].rerun == (n_fast++ ? true : rerun_all));
      for (int i = 0; i < pl.n_valu; ++i) {
        if (pl.valu[i].family != F::no_fit) CHECK(pl.valu[i].rerun == (n_fast++ ? true : rerun_all));
      }
      CHECK(pl.general_rerun == (rerun_all || n_fast > 0));
      CHECK(pl.p0_pass == (s.p0_valid ? 0 : (pl.general_rerun ? 2 : 1)));
      // 4. at most two VALU tiles, ascending; none when the tile-layout instances cover them
      CHECK(pl.n_valu <= 2 && (pl.n_valu < 2 || pl.valu[0].bs < pl.valu[1].bs));
      CHECK(!pl.mf_covers || (pl.n_valu == 0 && pl.n_mf > 0));
      // and: nothing fast beyond eight observables; a head within the batch, only on a first pass; tails only when wanted
      if (p > 8) CHECK(n_fast == 0 && pl.reserve_bytes == 0 && !pl.fold);
      for (int i = 0; i < pl.n_valu; ++i) {
        const KalmanPlan::Valu& v = pl.valu[i];
        CHECK(v.family != F::too_wide && v.bs >= 1 && v.bs <= 8 && v.s_cap >= 1 && v.s_cap <= 8 * v.bs);
        CHECK(v.head >= 0 && v.head <= c.batch && (v.head == 0 || (!v.rerun && v.family == F::nt && v.bs <= 4)));
        CHECK(!v.tail || (pl.want_tail && v.bs <= 4));
        CHECK(v.family != F::sel_tail || pl.want_tail);
      }
      CHECK(pl.n_tails <= 4 && (pl.n_tails == 0 || pl.want_tail));
      for (int i = 1; i < pl.n_tails; ++i) CHECK(pl.tails[i].m_lo == pl.tails[i - 1].mc && pl.tails[i].mc == pl.tails[i].m_lo + 8);
      CHECK(pl.general_bs == (m + 7) / 8);
    }
  }
  return n;
}

int main() {
  named_shapes();
  const long n = sweep();
  std::printf("kalman_plan_check: %ld plans swept, %d checks failed\n", n, g_failed);
  return g_failed ? 1 : 0;
}
