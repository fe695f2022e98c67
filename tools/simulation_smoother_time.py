"""GPU box: wall time (device events) of the simulation smoother on the SW-shaped workload (m = 40, k = 7, p = 7, T = 200).

    python tools/simulation_smoother_time.py [draws ...]          (default: 256 1024)

Per batch size, with device-resident inputs, draws and outputs, after a warm-up and over >= 1 s of timed work each:
  * LogpEngine.simulation_smoother with n_paths = 1 and with n_paths = 16 (x0, eps, eta given: no generation in the timed call),
  * LogpEngine.kalman_smoother without covariances on the same inputs -- the yardstick, in the same run: the simulation smoother
    contains its forward pass and basis, and its backward kernel is that smoother's mean half with 16 right-hand sides,
and the two ratios: one path / yardstick, sixteen paths / one path (16 would mean that nothing is shared)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oracle
from geconpy_amd import workloads as wl
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


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [256, 1024]
    eng = LogpEngine(0)
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, (T_len, p) = 40, 7, om["y"].shape
    Z, y, H = eng.to_device(om["Z"]), eng.to_device(om["y"]), eng.to_device(om["Hdiag"])
    print(f"SW shape m={m} k={k} p={p} T={T_len}")
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(1)
    for nb in sizes:
        rep = (nb + 63) // 64
        T = eng.to_device(np.tile(b["T_star"], (rep, 1, 1))[:nb])
        R = eng.to_device(np.tile(R64, (rep, 1, 1))[:nb])
        q = eng.to_device(np.tile(b["sigma"] ** 2, (rep, 1))[:nb])
        st = torch.zeros(nb, dtype=torch.int32, device=eng.device)
        times = {}
        for n_paths in (1, 16):
            d = eng.simulation_smoother(T, R, q, Z, y, n_paths=n_paths, Hdiag=H, q_mode=1, generator=gen, return_draws=True)
            torch.cuda.synchronize()
            assert int(d["status"].abs().max().item()) == 0 and bool(torch.isfinite(d["states"]).all().item())
            x0, eps, eta = d["x0"], d["eps"], d["eta"]
            del d
            times[n_paths] = timed(lambda: eng.simulation_smoother(T, R, q, Z, y, n_paths=n_paths, Hdiag=H, q_mode=1, x0=x0, eps=eps,
                                                                   eta=eta, status=st))
        t_y, n_y = timed(lambda: eng.kalman_smoother(T, R, q, Z, y, Hdiag=H, q_mode=1, covariances=False, status=st))
        assert int(st.abs().max().item()) == 0
        (t1, n1), (t16, n16) = times[1], times[16]
        print(f"draws={nb:5d} simulation smoother: 1 path {t1:9.3f} ms, 16 paths {t16:9.3f} ms; smoother without covariances "
              f"{t_y:9.3f} ms; 1 path / smoother {t1 / t_y:5.2f}, 16 paths / 1 path {t16 / t1:5.2f}")
        print(f"draws={nb:5d} calls timed: 1 path {n1}, 16 paths {n16}, smoother {n_y}")


if __name__ == "__main__":
    main()
