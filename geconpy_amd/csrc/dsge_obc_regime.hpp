// The regime iteration of the occasionally binding bound (dsge_obc.hpp), as one force-inlined function of a wavefront, and the
// constants its callers share: obc_regime_kernel (dsge_obc.hpp, one call per path) and obc_sim_kernel (dsge_obc_sim.hpp, one call per
// path and period).
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int OBC_THREADS = 256, OBC_WAVES = 4;  // paths (wavefronts) per workgroup
constexpr int OBC_MAX_H = 64;                     // DSGE_OBC_MAX_HORIZON
constexpr int OBC_NO_REGIME = 1, OBC_SINGULAR = 2, OBC_BEYOND = 4, OBC_SKIPPED = 8;  // DSGE_OBC_*
constexpr int OBC_FAILED = OBC_NO_REGIME | OBC_SINGULAR | OBC_SKIPPED;
constexpr int OBC_ST_UNRESOLVED = 4096;           // DSGE_ST_CONSTRAINT_UNRESOLVED

// THE REGIME ITERATION of one path, by one wavefront: lane h holds q_h (h < H: act), Mz [H][ld] is the draw's in the LDS, nub [64]
// the wavefront's own slot.  HM: 32 or 64, the rows of K a lane holds.  Returns the path's bits (0, OBC_SINGULAR or OBC_NO_REGIME);
// nu: lane h's nu_h (the caller's value stays when q is not finite), S: the last binding set, iters: the solves, added to the
// caller's count.  On return nub holds nu when S is not empty (and is untouched when it is)
template <int HM>
__device__ __forceinline__ int obc_regime_iterate(const ks_lds* Mz, int ld, ks_lds* nub, int lane, bool act, double q, double thr,
                                                  int max_iter, double& nu, int& iters, unsigned long long& S_out) {
  int st = 0;
  unsigned long long S = 0ull;
  if (__ballot(act && !(fabs(q) < INFINITY)) != 0ull) {
    st = OBC_SINGULAR;
  } else {
    S = __ballot(act && q < 0.0);
    for (;;) {
      ++iters;
      nu = 0.0;
      const bool in_s = (S >> lane) & 1ull;
      if (S != 0ull) {
        double kr[HM];
#pragma unroll
        for (int c = 0; c < HM; ++c) kr[c] = in_s && ((S >> c) & 1ull) ? Mz[lane * ld + c] : 0.0;
        double rhs = in_s ? -q : 0.0, pv = 1.0;
        unsigned long long avail = S;  // rows that have not been a pivot row
        int mycol = lane;              // the column whose solution this row ends up holding
        bool singular = false;
#pragma unroll
        for (int j = 0; j < HM; ++j) {
          if (singular || !((S >> j) & 1ull)) continue;  // (wave-uniform)
          double v = fabs(kr[j]);
          if (!(v == v)) v = INFINITY;  // a NaN wins, and fails the test below
          const unsigned long long key = (avail >> lane) & 1ull ? (unsigned long long)__double_as_longlong(v) : 0ull;
          const unsigned long long best = wave_max_u64(key);
          const unsigned long long who = __ballot(((avail >> lane) & 1ull) && key == best);
          const int r = __builtin_ctzll(who);  // (a row is left whenever a column of S is)
          const double piv = readlane_dyn_f64(kr[j], r);
          if (!(fabs(piv) > thr) || !(fabs(piv) < INFINITY)) {
            singular = true;
            continue;
          }
          avail &= ~(1ull << r);
          const bool is_r = lane == r;
          if (is_r) {
            mycol = j;
            pv = piv;
          }
          const double f = is_r ? 0.0 : kr[j] / piv;
#pragma unroll
          for (int c = j + 1; c < HM; ++c)
            if ((S >> c) & 1ull) kr[c] = fma(-f, readlane_dyn_f64(kr[c], r), kr[c]);
          rhs = fma(-f, readlane_dyn_f64(rhs, r), rhs);
        }
        if (singular) {
          st = OBC_SINGULAR;
          break;
        }
        // row r holds the solution of column mycol; rows off S hold zero for their own column
        __builtin_amdgcn_wave_barrier();
        nub[mycol] = in_s ? rhs / pv : 0.0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        nu = nub[lane];
      }
      double gp = q;
      if (act)
        for (unsigned long long bits = S; bits != 0ull; bits &= bits - 1ull) {
          const int j = __builtin_ctzll(bits);
          gp = fma(Mz[lane * ld + j], nub[j], gp);
        }
      const unsigned long long Sn = __ballot(act && (in_s ? nu > 0.0 : gp < 0.0));
      if (Sn == S) break;
      if (iters >= max_iter) {
        st = OBC_NO_REGIME;
        break;
      }
      S = Sn;
    }
  }
  S_out = S;
  return st;
}

}  // namespace dsge
