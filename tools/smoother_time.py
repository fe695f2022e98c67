"""GPU box: wall time (device events) of the smoother on the SW-shaped workload (m = 40, k = 7, p = 7, T = 200).

    python tools/smoother_time.py [--rank-tol X] [draws ...]          (default: 256 1024)

(--rank-tol 2 stops the range basis at r = 1: wrong results, but the time that does not depend on r.)

Per batch size, with device-resident inputs and outputs, after a warm-up and over >= 1 s of timed work each:
  * LogpEngine.kalman_smoother with diagonal covariances,
  * the same without covariances (the G / V work is skipped),
  * dsge_kalman_filter_outputs_batched with full covariances on the same inputs -- the yardstick: the most comparable call
    without the smoother, and the smoother contains it (forward pass into library scratch).
and the FP64 flops of one backward step counted from the shapes, with the rate they imply for the backward pass when its time is
taken as (smoother - yardstick) -- an estimate: basis kernel and assembly are in that difference too; a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/smoother_time.py 256) gives kalman_smoother_kernel's own time."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oracle
from geconpy_amd import _lib, workloads as wl
from geconpy_amd.engine import LogpEngine


def timed(fn, min_seconds=1.0):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
        reps += 4
    return total / reps * 1e3, reps  # ms per call


def backward_flops_per_step(m, r, k, cov):
    vec = 2 * m * r * 2 + 2 * r * r + 2 * m * m * 2 + 2 * m * k  # U'd, U z, triangular solves, T'w, P_filt (T'w), R'w
    f = 2 * m * m * r + 2 * m * r * r + r ** 3 / 3 + vec          # E = Pp U, M = U'E, Cholesky
    if cov:
        f += 2 * r * m * m + 2 * r * r * m + 2 * m * m * r + 4 * m ** 3  # C, M^-1 C, G' = U X, F = D G', S = G F
    return f


def main():
    argv = sys.argv[1:]
    rank_tol = None
    if "--rank-tol" in argv:
        i = argv.index("--rank-tol")
        rank_tol = float(argv[i + 1])
        del argv[i:i + 2]
    sizes = [int(a) for a in argv] or [256, 1024]
    eng = LogpEngine(0)
    lib = _lib.load()
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, (T_len, p) = 40, 7, om["y"].shape
    r = int(np.linalg.matrix_rank(np.concatenate([b["T_star"][0], R64[0]], axis=1), tol=1e-10))
    Z, y, H = eng.to_device(om["Z"]), eng.to_device(om["y"]), eng.to_device(om["Hdiag"])
    if rank_tol is not None:
        print(f"rank_tol = {rank_tol}: the basis is NOT that of [T|R]; flop counts below assume r = {r}")
    print(f"SW shape m={m} k={k} p={p} T={T_len}, rank of [T|R] = {r}; counted flops per backward step: "
          f"{backward_flops_per_step(m, r, k, True):.0f} with covariances, {backward_flops_per_step(m, r, k, False):.0f} without")
    for nb in sizes:
        rep = (nb + 63) // 64
        T = eng.to_device(np.tile(b["T_star"], (rep, 1, 1))[:nb])
        R = eng.to_device(np.tile(R64, (rep, 1, 1))[:nb])
        q = eng.to_device(np.tile(b["sigma"] ** 2, (rep, 1))[:nb])
        mk = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)  # noqa: E731
        ll, ap, af, pp, pf = mk(nb, T_len), mk(nb, T_len, m), mk(nb, T_len, m), mk(nb, T_len, m, m), mk(nb, T_len, m, m)
        st = torch.zeros(nb, dtype=torch.int32, device=eng.device)

        def yardstick():
            _lib.check(lib.dsge_kalman_filter_outputs_batched(
                T.data_ptr(), R.data_ptr(), q.data_ptr(), 1, Z.data_ptr(), 0, None, 0, H.data_ptr(), 0, y.data_ptr(), nb, m, k, p,
                T_len, 1e-8, -9999.0, ll.data_ptr(), ap.data_ptr(), af.data_ptr(), pp.data_ptr(), pf.data_ptr(), 1, st.data_ptr(),
                eng._stream()))

        def smoother(cov):
            return lambda: eng.kalman_smoother(T, R, q, Z, y, Hdiag=H, q_mode=1, covariances=cov, status=st, rank_tol=rank_tol)

        t_y, n_y = timed(yardstick)
        t_d, n_d = timed(smoother(True))
        t_n, n_n = timed(smoother(False))
        assert int(st.abs().max().item()) == 0
        for name, t_s, cov in (("diagonal covariances", t_d, True), ("no covariances", t_n, False)):
            fl = backward_flops_per_step(m, r, k, cov) * (T_len - 1) * nb
            print(f"draws={nb:5d} smoother, {name:21s}: {t_s:9.3f} ms  (yardstick {t_y:8.3f} ms, ratio {t_s / t_y:5.2f}; "
                  f"backward ~ {t_s - t_y:8.3f} ms -> {fl / max(t_s - t_y, 1e-9) * 1e-9:7.3f} TFLOP/s counted)")
        print(f"draws={nb:5d} calls timed: yardstick {n_y}, diagonal {n_d}, none {n_n}")


if __name__ == "__main__":
    main()
