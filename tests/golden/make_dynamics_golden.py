"""Container-only: tests/golden/dynamics_reference.npz -- what the reference's own simulation loop gives on two real models.

``_simulate_linear_system`` (gEconpy/model/simulate.py) is taken out of the reference file by AST at run time, the way
``_ref_extract.py`` does it for the solvers (the function needs numpy alone); nothing of its text is copied.  For
``workloads.rbc_batch`` (m = 8, k = 1) and ``workloads.full_nk_batch`` (m = 24, k = 4) the fixture holds draw 0's T and R
(the oracle's cycle reduction at tol 1e-12 + compute_selection_matrix), the unit-impulse responses over 40 periods (one call
per shock, as ``impulse_response_function`` makes them) and one trajectory-mode run with a fixed 12 x k shock matrix.

    python tests/golden/make_dynamics_golden.py
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle  # noqa: E402
from oracle.cycle_reduction import cycle_reduction_core  # noqa: E402
from geconpy_amd import workloads as wl  # noqa: E402

REF = os.environ.get("GECONPY_REFERENCE", "/root/reference")


def reference_loop():
    path = os.path.join(REF, "gEconpy", "model", "simulate.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_simulate_linear_system"]
    assert len(keep) == 1
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, path, "exec"), ns)
    return ns["_simulate_linear_system"]


def main():
    sim = reference_loop()
    out = {}
    for name, make in (("rbc", wl.rbc_batch), ("full_nk", wl.full_nk_batch)):
        b, _ = make(1)
        A, B, C, D = (b[x][0] for x in "ABCD")
        T, ok, _ = cycle_reduction_core(A, B, C, 1000, 1e-12)
        assert ok
        R = oracle.compute_selection_matrix(B, C, D, T)
        k = R.shape[1]
        irf = np.empty((k, 40, T.shape[0]))
        for j in range(k):
            traj = np.zeros((40, k))
            traj[0, j] = 1.0
            irf[j] = sim(T, R, traj)
        shocks = np.random.default_rng(11).normal(0.0, 1.0, (12, k))
        out.update({f"{name}_T": T, f"{name}_R": R, f"{name}_irf": irf, f"{name}_shocks": shocks,
                    f"{name}_path": sim(T, R, shocks)})
    np.savez_compressed(os.path.join(HERE, "dynamics_reference.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
