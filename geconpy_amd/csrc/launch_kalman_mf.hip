// Launcher of the tile-layout filter kernel (dsge_kalman_mf.hpp): its own translation unit -- seven template instances, compiled
// next to launch_kalman.hip instead of inside it.
#include "dsge_kalman_launch.hpp"
#include "dsge_kalman_plan.hpp"

namespace dsge_host {

// The covariance in the tile layout of the FP64 matrix core's 4 x 4 x 4 instruction -- downdate and both prediction products as matrix
// issues (63 per full step on the SW-shaped model).  One instance of the plan (kalman_plan chooses them from the caller's hint and
// checks that the staged R fits): the kernel checks every draw and flags what does not fit (DSGE_ST_INTERNAL_RERUN) for the next
// instance.  What these instances refuse -- more state variables than the hint, a design matrix that is no selector -- the VALU
// fast kernels refuse too (their state-block capacity comes from the same hint, and with s <= 20, p <= 8 no draw has more than 28
// retained variables): when the plan's instances cover them, their empty second passes (~5 us each) are skipped and a refused draw
// goes straight to the general kernel.  dsge_options.kalman_mfma = 2 (default); 0: the VALU kernels.
int launch_kalman_mf(const KalmanPlan::Mf& f, FilterArgs a, hipStream_t st) {
  a.rerun = f.rerun;
  switch (10 * f.kt + f.tm) {
    case 33: return launch_mf<3, 3, false>(a.batch, st, f.lds, a);
    case 35: return launch_mf<3, 5, false>(a.batch, st, f.lds, a);
    case 44: return launch_mf<4, 4, false>(a.batch, st, f.lds, a);
    case 46: return launch_mf<4, 6, false>(a.batch, st, f.lds, a);
    case 57: return launch_mf<5, 7, false>(a.batch, st, f.lds, a);
    case 55:  // (tools/kalman_phases.py: the stamped instance of the SW-shaped size)
      return f.stamped ? launch_mf<5, 5, true>(a.batch, st, f.lds, a) : launch_mf<5, 5, false>(a.batch, st, f.lds, a);
  }
  return fail(DSGE_ERR_INVALID, "launch_kalman_mf: no such instance");
}

}  // namespace dsge_host
