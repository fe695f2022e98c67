"""GPU box: what the refinement branch of the cycle reduction costs the headline step (4096 SW-shaped draws through the fused
likelihood call), measured with dsge_debug_cr_refine: mode 0 = the rule, mode 1 = the instance without the branch (RESULTS CHANGE
on the draws that would have refined: a measuring tool, nothing else uses mode 1).

    python tools/cr_refine_cost.py [batch] [steps]     five alternating runs per mode, ms per step, and the draws whose logp moves
    python tools/cr_refine_cost.py trace MODE [batch]  105 steps under one mode, for a kernel trace of its own
"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from geconpy_amd import _lib, workloads as wl
from geconpy_amd.engine import LogpEngine

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
args = sys.argv[3:] if trace else sys.argv[1:]
nb = int(args[0]) if len(args) > 0 else 4096
steps = 100 if trace else (int(args[1]) if len(args) > 1 else 800)
b = wl.sw_shaped_batch(nb)
om = wl.sw_shaped_observation_model()
eng = LogpEngine(0)
lib = _lib.load()
dev = [eng.to_device(b[x]) for x in "ABCD"]
dq = eng.to_device(b["sigma"] ** 2)
dZ, dy, dH = eng.to_device(om["Z"]), eng.to_device(om["y"]), eng.to_device(om["Hdiag"])
ns, zs = eng.structure_hints(dev[0], dZ)
opts = {"n_static_hint": eng.static_hint(dev[0], dev[2])}
lp = torch.empty(nb, dtype=torch.float64, device="cuda")
st = torch.empty(nb, dtype=torch.int32, device="cuda")


def step():
    eng.solve_kalman_logp(*dev, dq, dZ, dy, Hdiag=dH, q_mode=1, tol=1e-8, max_iter=1000, logp=lp, status=st, n_state_hint=ns,
                          z_selector_hint=zs, options=opts)


def run(mode, n):
    _lib.check(lib.dsge_debug_cr_refine(mode))
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


try:
    if trace:
        print("mode", int(sys.argv[2]), "%.4f ms per step" % run(int(sys.argv[2]), steps))
    else:
        ms = {0: [], 1: []}
        out = {}
        for _ in range(5):
            for mode in (0, 1):
                ms[mode].append(run(mode, steps))
                out[mode] = (lp.cpu().numpy().copy(), st.cpu().numpy().copy())
        for mode in (0, 1):
            v = ms[mode]
            print("mode %d  " % mode + "  ".join("%.4f" % x for x in v) + "    median %.4f   max - min %.4f" % (np.median(v), max(v) - min(v)))
        print("mode 1 - mode 0 (medians): %.4f ms" % (np.median(ms[1]) - np.median(ms[0])))
        moved = np.flatnonzero(out[0][0] != out[1][0])
        rel = np.abs(out[0][0][moved] - out[1][0][moved]) / np.abs(out[0][0][moved])
        print("draws whose logp differs between the modes:", len(moved), "of", nb, moved[:40].tolist(), "largest relative difference",
              rel.max() if len(moved) else 0.0, "status differs on", int((out[0][1] != out[1][1]).sum()))
finally:
    _lib.check(lib.dsge_debug_cr_refine(0))
