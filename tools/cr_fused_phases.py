"""GPU box: per-phase shader cycles of the fused deflation + cycle-reduction launch (draw 0 inside a batch of SW-shaped draws),
from the stamped instance cr_fused_kernel_occ2_dbg<5, 4> (dsge_debug_cr_fused_phases): python tools/cr_fused_phases.py [batch] [distinct]
Default: 64 distinct draws tiled to the batch; `distinct`: the bench's batch (sw_shaped_batch(batch), every draw its own), which is
what the refinement counts of the last lines are about -- they are summed over every draw of the batch, not taken from draw 0."""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from geconpy_amd import _lib, batched, workloads as wl
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
distinct = len(sys.argv) > 2 and sys.argv[2] == "distinct"
b = wl.sw_shaped_batch(nb if distinct else min(nb, 64))
om = wl.sw_shaped_observation_model()
rep = 1 if distinct else (nb + 63) // 64
t = {x: np.tile(b[x], (rep,) + (1,) * (b[x].ndim - 1))[:nb] for x in ("A", "B", "C", "D", "sigma")}
lib = _lib.load()
_lib.check(lib.dsge_debug_cr_fused_phases(1, None))
CALLS = 2
for _ in range(CALLS):
    r = batched.solve_kalman_logp_batched(t["A"], t["B"], t["C"], t["D"], t["sigma"] ** 2, om["Z"], om["y"], Hdiag=om["Hdiag"],
                                          q_mode=1, tol=1e-8, max_iter=1000, options={"n_static_hint": batched.static_hint(t["A"][:1], t["C"][:1])})
cyc = (ctypes.c_longlong * 24)()
_lib.check(lib.dsge_debug_cr_fused_phases(0, ctypes.addressof(cyc)))
c = np.array(list(cyc)); it = max(int(c[7]), 1)
assert (r["status"] == 0).all() and c[6] > 0, "the stamped instance did not run (not the 40 -> 30 variable shape?)"
names = ["GJ panels", "GJ trailing", "gather+stage", "products", "scatter+norms"]
print("iterations", int(c[7]), "total", int(c[6]))
print("phase 1: loads+scans", int(c[8]), "reflectors", int(c[9]), "deposit", int(c[10]))
print("iterations, all:", int(c[:5].sum()), "per iteration:", {n: int(v / it) for n, v in zip(names, c[:5])})
print("final solve", int(c[5]), "phase 3", int(c[11]), "unstamped rest", int(c[6] - c[:6].sum() - c[8:12].sum()))
print("loads+scans: static mask", int(c[12]), "tables + column loads", int(c[8] - c[12]))
print("phase 3: gather of y", int(c[13]), "inflate_prepare", int(c[14]), "inflate_chunk", int(c[15]),
      "zero + scatter stores", int(c[11] - c[13:16].sum()))
# the refinement branch, over the whole batch (the counters add up over the CALLS launches)
assert (c[[16, 17, 21, 22, 23]] % CALLS == 0).all(), "the launches of one batch refine alike"
nref = max(int(c[17]), 1)
print("refinement: draws of the batch that refine", int(c[16]) // CALLS, "of", nb, "refinements", int(c[17]) // CALLS,
      "draws refining in 1 / 2 / 3+ iterations", [int(v) // CALLS for v in c[21:24]])
print("one refinement (average, cycles): residual", int(c[18] / nref), "second elimination", int(c[19] / nref),
      "stores + reordering", int((c[20] - c[18] - c[19]) / nref), "whole branch", int(c[20] / nref))
