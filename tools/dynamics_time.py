"""GPU box: wall time (device events) of the post-solve dynamics entries on the SW-shaped workload (m = 40, k = 7, 40 steps).

    python tools/dynamics_time.py [draws ...]          (default: 256 4096)
    python tools/dynamics_time.py --second-order [draws ...]      the second-order rows alone
    python tools/dynamics_time.py --decomposition [draws ...]     the shock-decomposition rows alone
    python tools/dynamics_time.py --conditional [draws ...]       the conditional-forecast rows alone
    python tools/dynamics_time.py --spectral [draws ...]          the spectral-moments rows alone
    python tools/dynamics_time.py --anticipated [draws ...]       the anticipated-shock rows alone
    python tools/dynamics_time.py --constrained [draws ...]       the occasionally-binding-bound rows alone
    python tools/dynamics_time.py --stochastic-bound [draws ...]  the rows of the stochastic simulation at the bound alone
    python tools/dynamics_time.py --segmented [draws ...]         the rows of the Kalman likelihood across dated breaks alone
    python tools/dynamics_time.py --segmented-smoother [--library PATH] [--scratch-limit-gib G] [draws ...]   the smoother across breaks
    python tools/dynamics_time.py --segmented-gradient [--library PATH] [--scratch-limit-gib G] [draws ...]   the gradient across breaks

Per batch size, with device-resident inputs and outputs, after a warm-up and over >= 1 s of timed work each:
  * LogpEngine.impulse_response (unit impulses, c = 7) and LogpEngine.simulate (16 paths, shocks at every step), each against a
    plain device fill (torch's fill_) of an array the size of its output, timed in the same run -- the yardstick: the kernel
    writes each output byte once and reads almost nothing; the implied write rate is printed next to both;
  * the impulse responses with the on-chip FEVD;
  * LogpEngine.forecast with full covariances (p = 0) against dsge_kalman_filter_outputs_batched with full covariances at
    T_len = 40 on the same draws -- per step the forecast does that kernel's two covariance products and none of its update;
  * the same two jobs as a host numpy loop over the draws (tests' restatement), for the CPU comparison;
  * second order (csrc/dsge_pruned.hpp), n = 40, s = 18, k = 7: LogpEngine.simulate_pruned (16 paths) next to the first-order
    LogpEngine.simulate on the same T, R and shocks in the same run -- the yardstick of the ratio is the K-extent of a step's
    products, 48 against 48 + 48 + 336 -- then LogpEngine.girf_pruned (7 unit impulses over 16 baseline paths) and the host numpy
    loop of tests/pruned_dynamics_reference.py (256 draws timed once, scaled).
  * --decomposition (csrc/dsge_shock_decomp.hpp), m = 40, k = 7, identity groups, all 40 variables, T_len = 200: the median of five
    timings of >= 1 s each of LogpEngine.shock_decomposition (with and without the remainder), of the composed route that was the
    only one before it -- LogpEngine.simulate with k + 1 paths on an expanded shock array, the expansion by torch timed apart; it
    still lacks the transpose and the remainder -- and of a plain fill of the output array.
  * --conditional (csrc/dsge_condfc.hpp), m = 40, k = 7, p = 7 (selector Z): observables 0, 2, 4 conditioned over 12 periods (36
    conditions), all shocks free, 40 steps, 16 paths with baseline shocks at every step: the median of five timings of >= 1 s each
    of LogpEngine.conditional_forecast and of the composed route that was the only one before it -- LogpEngine.simulate (the
    baseline), LogpEngine.impulse_response (12 steps: Psi), the torch algebra (gather of W, Gram matrix, linalg.cholesky,
    cholesky_solve, the corrected shocks) and a second LogpEngine.simulate -- each part also timed apart; then the phase stamps of
    one call (dsge_debug_condfc_phases).
  * --spectral (csrc/dsge_spectral.hpp), m = 40, k = 7, p = 7 (selector Z), N = 512 (257 frequencies), n_lags = 10, HP gain,
    autocovariances only: the median of five timings of >= 1 s each of LogpEngine.spectral_moments and of the composed route that
    was the only exact one before it -- torch.linalg.solve on the complex128 stack (draws x 257, 40, 40) (the real 80 x 80
    embedding in float64 if this torch has no complex batched solve on the device), the einsum for H Q H^H and the cosine / sine
    sums, chunked over 512 draws -- with its parts timed apart and the agreement of the two routes.
  * --anticipated (csrc/dsge_anticipated.hpp), the SW-shaped (B, C, T) with a dense impact matrix D = randn(n, k) / sqrt(n) and
    R = -(B + C T)^-1 D (on the generator's own D anticipation does nothing: tests/anticipated_cases.py), m = 40, k = 7, 40 steps, 16
    paths: the median of five timings of >= 1 s each of LogpEngine.anticipated_paths -- perfect foresight with shocks at every step,
    and news with n_lead = 4 -- and of the composed route that was the only one before it: torch.linalg.solve for G, a bmm loop
    for w (backward over the 40 periods; news: five Horner products on all periods at once) and LogpEngine.simulate with R = I;
    the parts timed apart, the setup kernel alone (outputs=("G",)), and the agreement of the two routes.
  * --constrained (csrc/dsge_obc.hpp), the model of --anticipated, 40 steps, 16 paths with shocks at every step, the bound on
    the variable shock 0 moves most, at half the minimum of the draw's unconstrained paths, H = 32, x the only output: the median
    of five timings of >= 1 s each of LogpEngine.constrained_paths and of the composed route that was the only one before it --
    LogpEngine.anticipated_paths three times (the H unit paths observed through c for Mz, the unconstrained paths, the final paths
    on eps + nu e_s) around a torch loop of batched torch.linalg.solve on the identity-padded systems with the same updates of S,
    one host round trip per iteration -- with the agreement of the two routes, the parts of the entry timed apart through its own
    subsets of outputs and the anticipated-shock entry, and the mean and largest iters.
  * --segmented (csrc/dsge_kalman_seg.hpp), m = 40, k = 7, T_len = 200, p and Z of bench.py's workload: the median of five timings
    of >= 1 s each of LogpEngine.kalman_logp_segments with S = 1, S = 3 (breaks at 80 and 140) and S = 8, against
    dsge_kalman_filter_outputs_batched with ll alone and, for scale, dsge_kalman_logp_batched with kalman_steady_tol = 0 and at its
    default.
  * --segmented-smoother [--library PATH] [--scratch-limit-gib G] (docs/design/segmented_smoother.md), the batch of --segmented: the median of five timings
    of >= 1 s each of LogpEngine.kalman_smoother_segments (ll, smoothed states and shocks; with diagonal covariances and without
    covariances) with S = 1, S = 3 and S = 8, against dsge_kalman_smoother_batched on the inputs of S = 1 -- of this build and of
    the library at PATH (a build of another commit) in the same run -- with the cost per boundary and whether S = 1 has its bits.
  * --segmented-gradient [--library PATH] [--scratch-limit-gib G] (docs/design/segmented_gradient.md), the batch of --segmented: the
    median of five timings of >= 1 s each of LogpEngine.kalman_logp_segments_grad (every cotangent) with S = 1, S = 3 and S = 8, next
    to dsge_kalman_logp_segments_batched (logp alone) on the same inputs -- of the library at PATH (a build of the parent commit)
    loaded in the same process, else of this build -- with the ratio gradient / likelihood, whether logp has the likelihood's
    bits, and for scale the cost of the same gradient of T alone by central differences (stated, not run).
Kernel times proper: rocprofv3 --kernel-trace --stats -- python tools/dynamics_time.py 4096."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oracle
from geconpy_amd import _lib, workloads as wl
from geconpy_amd.engine import LogpEngine
from tests import dynamics_reference as dr

N_STEPS = 40


def timed(fn, min_seconds=1.0, warm=2, calls=4):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
        reps += calls
    return total / reps * 1e3  # ms per call


def second_order_rows(eng, sizes):
    from tests import pruned_dynamics_reference as pr

    c = pr.case("n40")
    nd, n, k = c["R"].shape
    s = len(c["S"])
    rng = np.random.default_rng(1)
    print(f"second order n={n} s={s} k={k}, {N_STEPS} steps, 16 paths")
    t_cpu = None
    for nb in sizes:
        rep = (nb + nd - 1) // nd
        sol = {key: eng.to_device(np.tile(c[key], (rep,) + (1,) * (c[key].ndim - 1))[:nb]) for key in pr.solution(c) if key != "S"}
        sol["S"] = c["S"]
        eps_h = rng.standard_normal((nb, 16, N_STEPS, k)) * 0.01
        eps = eng.to_device(eps_h)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        x, paths, girf = mk(nb, 16, N_STEPS, n), mk(nb, 16, N_STEPS, n), mk(nb, k, N_STEPS, n)
        t_first = timed(lambda: eng.simulate(sol["T"], sol["R"], eps, out=paths))
        t_sim = timed(lambda: eng.simulate_pruned(sol, eps, out=dict(x=x)))
        t_girf = timed(lambda: eng.girf_pruned(sol, N_STEPS, None, eps, out=girf))
        print(f"draws={nb:5d} simulate_pruned, 16 paths: {t_sim:8.3f} ms | first-order simulate, same run: {t_first:8.3f} ms | "
              f"ratio {t_sim / t_first:5.2f} (K-extent of the products: {(48 + 48 + 336) / 48:4.1f})")
        print(f"draws={nb:5d} girf_pruned, 7 impulses x 16 baseline paths: {t_girf:8.3f} ms")
        import ctypes

        lib, cyc = _lib.load(), (ctypes.c_longlong * 8)()  # per-phase shader cycles of wavefront 0 of workgroup 0, one call
        _lib.check(lib.dsge_debug_pruned_phases(1, None))
        eng.simulate_pruned(sol, eps, out=dict(x=x))
        _lib.check(lib.dsge_debug_pruned_phases(0, ctypes.addressof(cyc)))
        names = ("x_f product", "T x_s", "P mon", "barrier wait", "slab")
        print(f"draws={nb:5d} phases of one workgroup, cycles per step: "
              + ", ".join(f"{nm} {cyc[i] / max(cyc[6], 1):.0f}" for i, nm in enumerate(names))
              + f" | total {cyc[5]}, {cyc[6]} steps, set-up {cyc[7]}")
        if t_cpu is None:  # host numpy loop over 256 draws (or the batch, if smaller), scaled to the batch
            nc = min(nb, 256)
            t0 = time.perf_counter()
            for i in range(nc):
                T, R, so_ = pr.draw(c, i % nd)
                for p in range(16):
                    pr.simulate_pruned(T, R, so_, eps_h[i, p])
            t_cpu = (time.perf_counter() - t0) / nc * 1e3
            print(f"host numpy loop: {nc} draws timed, {t_cpu:8.2f} ms per draw")
        print(f"draws={nb:5d} host numpy loop (scaled): simulate_pruned {t_cpu * nb:9.1f} ms ({t_cpu * nb / t_sim:7.0f}x)")


def decomposition_rows(eng, sizes, T_len=200, repeats=5):
    b = wl.sw_shaped_batch(64)
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k = 40, 7
    rng = np.random.default_rng(0)
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    print(f"shock decomposition m={m} k={k}, identity groups, all variables, T_len={T_len}; medians of {repeats} timings of >= 1 s")
    for nb in sizes:
        rep = (nb + 63) // 64
        T, R = eng.to_device(np.tile(b["T_star"], (rep, 1, 1))[:nb]), eng.to_device(np.tile(R64, (rep, 1, 1))[:nb])
        e = eng.to_device(rng.standard_normal((nb, T_len, k)) * 0.01)
        e[:, 0] = float("nan")
        x0 = eng.to_device(rng.standard_normal((nb, m)) * 0.05)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        # the composed route: path j < k carries shock j alone, path k the initial condition; steps 1 .. T_len-1
        ex, x0e, paths = torch.zeros(nb, k + 1, T_len - 1, k, dtype=torch.float64, device=eng.device), mk(nb, k + 1, m).zero_(), mk(nb, k + 1, T_len - 1, m)
        x0e[:, k] = x0

        def expand():
            ex[:, :k] = torch.diag_embed(e[:, 1:]).permute(0, 2, 1, 3)

        expand()
        eng.simulate(T, R, ex, x0=x0e, out=paths)
        x = torch.cat([x0[:, None], paths.sum(dim=1)], dim=1).contiguous()  # a path with a rounding-size remainder
        full, bare = dict(contributions=mk(nb, T_len, m, k + 2)), dict(contributions=mk(nb, T_len, m, k + 1))
        eng.shock_decomposition(T, R, x, e, out=full)
        eng.shock_decomposition(T, R, x, e, remainder=False, out=bare)
        diff = (bare["contributions"][:, 1:] - paths.permute(0, 2, 3, 1)).abs().max().item()
        rem = full["contributions"][..., -1].abs().max().item()
        print(f"draws={nb:5d} entry against the composed route: max difference {diff:.1e}; remainder {rem:.1e} (max|x| {x.abs().max().item():.2f})")
        t_full = med(lambda: eng.shock_decomposition(T, R, x, e, out=full))
        t_bare = med(lambda: eng.shock_decomposition(T, R, x, e, remainder=False, out=bare))
        t_sim = med(lambda: eng.simulate(T, R, ex, x0=x0e, out=paths))
        t_exp = med(expand)
        t_fill = med(lambda: full["contributions"].fill_(1.0))
        gb = full["contributions"].numel() * 8e-9
        print(f"draws={nb:5d} shock_decomposition: {t_full:8.3f} ms = {gb / t_full:5.2f} TB/s written | without the remainder {t_bare:8.3f} ms | "
              f"composed route: simulate, {k + 1} paths {t_sim:8.3f} ms + expansion {t_exp:8.3f} ms | fill of the output {t_fill:8.3f} ms | "
              f"entry / simulate {t_full / t_sim:5.2f}, entry / fill {t_full / t_fill:5.2f}")
        import ctypes

        lib, cyc = _lib.load(), (ctypes.c_longlong * 8)()  # per-phase shader cycles of wavefront 0 of workgroup 0, one call
        _lib.check(lib.dsge_debug_shock_decomp_phases(1, None))
        eng.shock_decomposition(T, R, x, e, out=full)
        _lib.check(lib.dsge_debug_shock_decomp_phases(0, ctypes.addressof(cyc)))
        names = ("loads' issue + product", "wait for the loads + LDS stores", "barrier wait", "outputs")
        print(f"draws={nb:5d} phases of one workgroup, cycles per step: "
              + ", ".join(f"{nm} {cyc[i] / max(cyc[5], 1):.0f}" for i, nm in enumerate(names))
              + f" | total {cyc[4]}, {cyc[5]} steps, set-up and period 0 {cyc[6]}")


def conditional_rows(eng, sizes, n_steps=N_STEPS, n_paths=16, periods=12, series=(0, 2, 4), repeats=5):
    import ctypes

    b = wl.sw_shaped_batch(64)
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p = 40, 7, 7
    rng = np.random.default_rng(0)
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    ct = np.repeat(np.arange(periods), len(series)).astype(np.int32)
    cj = np.tile(np.array(series), periods).astype(np.int32)
    n_cond = len(ct)
    print(f"conditional forecast m={m} k={k} p={p}, {n_cond} conditions (series {list(series)} over {periods} periods), all shocks free, "
          f"{n_steps} steps, {n_paths} paths; medians of {repeats} timings of >= 1 s")
    # W[c, s k + f] = Psi[t_c - s, series index of c, f] for s <= t_c: the gather of the composed route, built once on the host
    sidx = np.tile(np.arange(len(series)), periods)
    s_ = np.arange(periods)[None, :, None]
    lag = ct[:, None, None] - s_
    gather = ((np.clip(lag, 0, None) * len(series) + sidx[:, None, None]) * k + np.arange(k)[None, None, :]).reshape(n_cond, periods * k)
    mask = np.broadcast_to(lag >= 0, (n_cond, periods, k)).reshape(n_cond, periods * k).astype(np.float64)
    for nb in sizes:
        rep = (nb + 63) // 64
        T, R = eng.to_device(np.tile(b["T_star"], (rep, 1, 1))[:nb]), eng.to_device(np.tile(R64, (rep, 1, 1))[:nb])
        sigma = np.tile(b["sigma"], (rep, 1))[:nb]
        Q, Z = eng.to_device(sigma ** 2), eng.to_device(np.eye(p, m))
        eps = eng.to_device(rng.standard_normal((nb, n_paths, n_steps, k)) * sigma[:, None, None, :])
        x0 = eng.to_device(rng.standard_normal((nb, n_paths, m)) * 0.05)
        vals = eng.to_device(rng.standard_normal((nb, n_paths, n_cond)) * 0.02)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        out = dict(x=mk(nb, n_paths, n_steps, m), shocks=mk(nb, n_paths, n_steps, k), observed=mk(nb, n_paths, n_steps, p))
        status = torch.zeros(nb, dtype=torch.int32, device=eng.device)
        entry = lambda: eng.conditional_forecast(T, R, Q, x0, (ct, cj, vals), n_steps, Z=Z, eps=eps, q_mode="diag_batched",  # noqa: E731
                                                 status=status, out=out)
        # the composed route
        base, irf, paths, eps2 = mk(nb, n_paths, n_steps, m), dict(irf=mk(nb, k, periods, m)), mk(nb, n_paths, n_steps, m), eps.clone()
        g_idx, g_mask = torch.as_tensor(gather, device=eng.device), eng.to_device(mask)
        obs_idx = torch.as_tensor(np.array(series), device=eng.device)
        ct_d, sj_d = torch.as_tensor(ct.astype(np.int64), device=eng.device), torch.as_tensor(cj.astype(np.int64), device=eng.device)
        sim1 = lambda: eng.simulate(T, R, eps, x0=x0, out=base)  # noqa: E731
        imp = lambda: eng.impulse_response(T, R, n_steps=periods, out=irf)  # noqa: E731

        def algebra():
            psi = irf["irf"][:, :, :, obs_idx].permute(0, 2, 3, 1).reshape(nb, -1)  # [l][series][f]
            W = psi[:, g_idx] * g_mask  # (nb, n_cond, periods k)
            WQ = W * Q.repeat(1, periods)[:, None, :]
            L = torch.linalg.cholesky(WQ @ W.transpose(1, 2))
            r = vals - base[:, :, ct_d, sj_d]  # (nb, n_paths, n_cond); selector Z, d = 0
            lam = torch.cholesky_solve(r.transpose(1, 2), L)  # (nb, n_cond, n_paths)
            delta = (WQ.transpose(1, 2) @ lam).transpose(1, 2).reshape(nb, n_paths, periods, k)
            eps2.copy_(eps)
            eps2[:, :, :periods] += delta

        sim2 = lambda: eng.simulate(T, R, eps2, x0=x0, out=paths)  # noqa: E731

        def composed():
            sim1()
            imp()
            algebra()
            sim2()

        entry()
        composed()
        torch.cuda.synchronize()
        assert int(status.abs().max()) == 0
        diff = (out["x"] - paths).abs().max().item() / paths.abs().max().item()
        miss = (out["observed"][:, :, ct_d, sj_d] - vals).abs().max().item() / paths.abs().max().item()
        print(f"draws={nb:5d} entry against the composed route: {diff:.1e} of max|x|; conditions missed by {miss:.1e} of max|x|")
        t_entry, t_comp = med(entry), med(composed)
        t_s1, t_imp, t_alg, t_s2 = med(sim1), med(imp), med(algebra), med(sim2)
        print(f"draws={nb:5d} conditional_forecast: {t_entry:8.3f} ms | composed route {t_comp:8.3f} ms = simulate {t_s1:8.3f} + "
              f"impulse_response {t_imp:8.3f} + torch algebra {t_alg:8.3f} + simulate {t_s2:8.3f} (sum {t_s1 + t_imp + t_alg + t_s2:8.3f}) | "
              f"entry / composed {t_entry / t_comp:5.2f}")
        lib, cyc = _lib.load(), (ctypes.c_longlong * 8)()  # per-phase shader cycles of wavefront 0 of workgroup 0 of both kernels, one call
        _lib.check(lib.dsge_debug_condfc_phases(1, None))
        entry()
        _lib.check(lib.dsge_debug_condfc_phases(0, ctypes.addressof(cyc)))
        names = ("setup: lags", "setup: G", "setup: Cholesky", "paths: loads + pass 1", "paths: solves", "paths: Delta", "paths: pass 2",
                 "paths: total")
        print(f"draws={nb:5d} phases of workgroup 0, cycles: " + ", ".join(f"{nm} {cyc[i]}" for i, nm in enumerate(names)))


def spectral_rows(eng, sizes, n_grid=512, n_lags=10, chunk=512, repeats=5):
    from geconpy_amd import batched

    b = wl.sw_shaped_batch(64)
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p, nf = 40, 7, 7, n_grid // 2 + 1
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    dev = eng.device
    g_h = batched.hp_gain(n_grid)
    gain, Z = eng.to_device(g_h), eng.to_device(np.eye(p, m))
    w = 2.0 * np.pi * np.arange(nf) / n_grid
    z = torch.as_tensor(np.exp(-1j * w), device=dev)  # (nf,)
    cn = np.where((np.arange(nf) == 0) | (2 * np.arange(nf) == n_grid), 1.0, 2.0)
    wts = torch.as_tensor(cn * g_h * np.exp(1j * np.outer(np.arange(n_lags + 1), w)) / n_grid, device=dev)  # (lags, nf)
    eye = torch.eye(m, dtype=torch.complex128, device=dev)
    try:
        torch.linalg.solve(eye[None].repeat(2, 1, 1), eye[None, :, :k].repeat(2, 1, 1))
        complex_solve = True
    except RuntimeError:
        complex_solve = False
    print(f"spectral moments m={m} k={k} p={p} (selector), N={n_grid} ({nf} frequencies), n_lags={n_lags}, HP gain, acov only; "
          f"medians of {repeats} timings of >= 1 s; composed route: {'complex128' if complex_solve else 'real 2m x 2m'} batched solve, "
          f"{chunk} draws per chunk")
    for nb in sizes:
        rep = (nb + 63) // 64
        T, R = eng.to_device(np.tile(b["T_star"], (rep, 1, 1))[:nb]), eng.to_device(np.tile(R64, (rep, 1, 1))[:nb])
        Q = eng.to_device((np.tile(b["sigma"], (rep, 1))[:nb]) ** 2)
        status = torch.zeros(nb, dtype=torch.int32, device=dev)
        out = dict(acov=torch.empty(nb, n_lags + 1, p, p, dtype=torch.float64, device=dev))
        entry = lambda: eng.spectral_moments(T, R, Q, n_grid=n_grid, n_lags=n_lags, Z=Z, gain=gain, q_mode="diag_batched",  # noqa: E731
                                             status=status, out=out)
        acov2 = torch.empty_like(out["acov"])
        Hbuf = torch.empty(min(nb, chunk), nf, p, k, dtype=torch.complex128, device=dev)

        def solve(c0, c1):
            Tc, Rc = T[c0:c1], R[c0:c1]
            if complex_solve:
                A = eye - z[None, :, None, None] * Tc[:, None]
                X = torch.linalg.solve(A, Rc[:, None].to(torch.complex128).expand(-1, nf, -1, -1))
            else:  # [[Ar, -Ai], [Ai, Ar]] [Xr; Xi] = [R; 0]
                Ar = torch.eye(m, dtype=torch.float64, device=dev) - z.real[None, :, None, None] * Tc[:, None]
                Ai = -z.imag[None, :, None, None] * Tc[:, None]
                A2 = torch.cat([torch.cat([Ar, -Ai], dim=-1), torch.cat([Ai, Ar], dim=-1)], dim=-2)
                B2 = torch.cat([Rc, torch.zeros_like(Rc)], dim=-2)[:, None].expand(-1, nf, -1, -1)
                X2 = torch.linalg.solve(A2, B2)
                X = torch.complex(X2[..., :m, :], X2[..., m:, :])
            Hbuf[: c1 - c0] = X[:, :, :p]  # selector Z

        def sums(c0, c1):
            H = Hbuf[: c1 - c0]
            F = torch.einsum("bnik,bk,bnjk->bnij", H, Q[c0:c1].to(torch.complex128), H.conj())
            acov2[c0:c1] = torch.einsum("ln,bnij->blij", wts, F).real

        def composed(parts=(True, True)):
            for c0 in range(0, nb, chunk):
                c1 = min(nb, c0 + chunk)
                if parts[0]:
                    solve(c0, c1)
                if parts[1]:
                    sums(c0, c1)

        entry()
        composed()
        torch.cuda.synchronize()
        assert int(status.abs().max()) == 0
        scale = acov2[:, 0].abs().amax(dim=(1, 2))
        diff = ((out["acov"] - acov2).abs().amax(dim=(1, 2, 3)) / scale).max().item()
        print(f"draws={nb:5d} entry against the composed route: {diff:.1e} of max|acov[0]| per draw")
        t_entry, t_comp = med(entry), med(composed)
        t_solve, t_sums = med(lambda: composed((True, False))), med(lambda: composed((False, True)))
        print(f"draws={nb:5d} spectral_moments: {t_entry:8.3f} ms | composed route {t_comp:8.3f} ms = batched solve {t_solve:8.3f} + "
              f"einsums {t_sums:8.3f} (sum {t_solve + t_sums:8.3f}) | entry / composed {t_entry / t_comp:5.2f}")


def anticipated_rows(eng, sizes, n_steps=N_STEPS, n_paths=16, n_lead=4, repeats=5):
    b = wl.sw_shaped_batch(64)
    m, k = 40, 7
    rng = np.random.default_rng(0)
    D64 = rng.standard_normal((64, m, k)) / np.sqrt(m)
    R64 = np.stack([np.linalg.solve(b["B"][i] + b["C"][i] @ b["T_star"][i], -D64[i]) for i in range(64)])
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    print(f"anticipated paths m={m} k={k}, dense impact matrix, {n_steps} steps, {n_paths} paths, shocks at every step; news: n_lead={n_lead}; "
          f"medians of {repeats} timings of >= 1 s")
    for nb in sizes:
        rep = (nb + 63) // 64
        B, C, T, R = (eng.to_device(np.tile(a, (rep, 1, 1))[:nb]) for a in (b["B"], b["C"], b["T_star"], R64))
        eps = eng.to_device(rng.standard_normal((nb, n_paths, n_steps, k)) * 0.01)
        exp = eng.to_device(rng.standard_normal((nb, n_paths, n_steps, n_lead + 1, k)) * 0.01)
        x0 = eng.to_device(rng.standard_normal((nb, n_paths, m)) * 0.05)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        out, out_n, g_only = dict(x=mk(nb, n_paths, n_steps, m)), dict(x=mk(nb, n_paths, n_steps, m)), dict(G=mk(nb, m, m))
        status = torch.zeros(nb, dtype=torch.int32, device=eng.device)
        pf = lambda: eng.anticipated_paths(B, C, T, R, eps, x0=x0, status=status, out=out)  # noqa: E731
        news = lambda: eng.anticipated_paths(B, C, T, R, exp, mode="news", x0=x0, status=status, out=out_n)  # noqa: E731
        setup = lambda: eng.anticipated_paths(B, C, T, R, eps, status=status, outputs=("G",), out=g_only)  # noqa: E731
        # the composed route
        eye = torch.eye(m, dtype=torch.float64, device=eng.device).expand(nb, m, m).contiguous()
        hold, W, paths = {}, mk(nb, n_paths, n_steps, m), mk(nb, n_paths, n_steps, m)

        def solve():
            hold["G"] = torch.linalg.solve(torch.baddbmm(B, C, T), -C)

        def w_pf():
            G, w = hold["G"], None
            for t in range(n_steps - 1, -1, -1):  # (nb, m, n_paths) per period
                re = torch.bmm(R, eps[:, :, t].transpose(1, 2))
                w = re if w is None else torch.baddbmm(re, G, w)
                W[:, :, t] = w.transpose(1, 2)

        def w_news():
            G, acc = hold["G"], None
            for j in range(n_lead, -1, -1):  # all periods at once: (nb, m, n_paths n_steps)
                re = torch.bmm(R, exp[:, :, :, j].reshape(nb, n_paths * n_steps, k).transpose(1, 2))
                acc = re if acc is None else torch.baddbmm(re, G, acc)
            W.copy_(acc.transpose(1, 2).reshape(nb, n_paths, n_steps, m))

        sim = lambda: eng.simulate(T, eye, W, x0=x0, out=paths)  # noqa: E731

        def composed_pf():
            solve()
            w_pf()
            sim()

        def composed_news():
            solve()
            w_news()
            sim()

        pf()
        news()
        composed_pf()
        torch.cuda.synchronize()
        assert int(status.abs().max()) == 0
        d_pf = (out["x"] - paths).abs().max().item() / paths.abs().max().item()
        composed_news()
        torch.cuda.synchronize()
        d_news = (out_n["x"] - paths).abs().max().item() / paths.abs().max().item()
        print(f"draws={nb:5d} entry against the composed route: perfect foresight {d_pf:.1e}, news {d_news:.1e} of max|x|")
        t_pf, t_cpf, t_news, t_cnews = med(pf), med(composed_pf), med(news), med(composed_news)
        t_setup, t_solve, t_wpf, t_wnews, t_sim = med(setup), med(solve), med(w_pf), med(w_news), med(sim)
        print(f"draws={nb:5d} perfect foresight: {t_pf:8.3f} ms | composed route {t_cpf:8.3f} ms = linalg.solve {t_solve:8.3f} + bmm loop "
              f"{t_wpf:8.3f} + simulate(R = I) {t_sim:8.3f} (sum {t_solve + t_wpf + t_sim:8.3f}) | entry / composed {t_pf / t_cpf:5.2f}")
        print(f"draws={nb:5d} news, n_lead={n_lead}:   {t_news:8.3f} ms | composed route {t_cnews:8.3f} ms = linalg.solve {t_solve:8.3f} + Horner bmm "
              f"{t_wnews:8.3f} + simulate(R = I) {t_sim:8.3f} (sum {t_solve + t_wnews + t_sim:8.3f}) | entry / composed {t_news / t_cnews:5.2f}")
        print(f"draws={nb:5d} phase split of the entry: setup kernel alone {t_setup:8.3f} ms, paths kernel (entry - setup): perfect foresight "
              f"{t_pf - t_setup:8.3f} ms, news {t_news - t_setup:8.3f} ms")


def constrained_rows(eng, sizes, n_steps=N_STEPS, n_paths=16, horizon=32, shock=0, repeats=5):
    b = wl.sw_shaped_batch(64)
    m, k, H = 40, 7, horizon
    rng = np.random.default_rng(0)
    D64 = rng.standard_normal((64, m, k)) / np.sqrt(m)
    R64 = np.stack([np.linalg.solve(b["B"][i] + b["C"][i] @ b["T_star"][i], -D64[i]) for i in range(64)])
    var = np.argmax(np.abs(R64[:, :, shock]), axis=1)
    c64 = np.zeros((64, m))
    c64[np.arange(64), var] = np.sign(R64[np.arange(64), var, shock])
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    print(f"constrained paths m={m} k={k}, dense impact matrix, {n_steps} steps, {n_paths} paths, shocks at every step, H={H}, bound at half "
          f"the unconstrained minimum; medians of {repeats} timings of >= 1 s")
    for nb in sizes:
        rep = (nb + 63) // 64
        B, C, T, R = (eng.to_device(np.tile(a, (rep, 1, 1))[:nb]) for a in (b["B"], b["C"], b["T_star"], R64))
        c = eng.to_device(np.tile(c64, (rep, 1))[:nb])
        eps = eng.to_device(rng.standard_normal((nb, n_paths, n_steps, k)) * 0.01)
        x0 = eng.to_device(rng.standard_normal((nb, n_paths, m)) * 0.05)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        xu = eng.anticipated_paths(B, C, T, R, eps, x0=x0)["x"]
        bound = (0.5 * torch.einsum("bptn,bn->bpt", xu, c).amin(dim=(1, 2))).contiguous()
        out, out_nu = dict(x=mk(nb, n_paths, n_steps, m)), dict(nu=mk(nb, n_paths, H))
        entry = lambda: eng.constrained_paths(B, C, T, R, eps, c, bound, shock, H, x0=x0, out=out)  # noqa: E731
        to_nu = lambda: eng.constrained_paths(B, C, T, R, eps, c, bound, shock, H, x0=x0, outputs=("nu",), out=out_nu)  # noqa: E731
        # the composed route
        unit = torch.zeros(H, H, k, dtype=torch.float64, device=eng.device)
        unit[torch.arange(H), torch.arange(H), shock] = 1.0
        Zc = c.reshape(nb, 1, m).contiguous()
        o_mz, o_xu, o_x, g_only = dict(observed=mk(nb, H, H, 1)), dict(x=mk(nb, n_paths, H, m)), dict(x=mk(nb, n_paths, n_steps, m)), dict(G=mk(nb, m, m))
        eye = torch.eye(H, dtype=torch.float64, device=eng.device)
        hold = {}

        def mz_paths():
            eng.anticipated_paths(B, C, T, R, unit, n_steps=H, Z=Zc, outputs=("observed",), out=o_mz)

        def unconstrained():
            eng.anticipated_paths(B, C, T, R, eps, n_steps=H, x0=x0, out=o_xu)

        def regime_loop():
            Mz = o_mz["observed"][..., 0].transpose(1, 2)  # (nb, h, j)
            q = torch.einsum("bptn,bn->bpt", o_xu["x"], c) - bound[:, None, None]
            S, iters = q < 0.0, 0
            while True:
                iters += 1
                d = S.to(torch.float64)
                K = eye + d[..., :, None] * (Mz[:, None] - eye) * d[..., None, :]
                nu = torch.linalg.solve(K, (-q * d)[..., None])[..., 0]
                gap = q + torch.einsum("bhj,bpj->bph", Mz, nu)
                S_new = torch.where(S, nu > 0.0, gap < 0.0)
                if bool((S_new == S).all()) or iters >= 64:  # (the host round trip of every iteration)
                    break
                S = torch.where((S_new == S).all(dim=-1, keepdim=True), S, S_new)  # a path that has its regime keeps it
            hold["eps2"] = eps.clone()
            hold["eps2"][:, :, :H, shock] += nu
            hold["iters"] = iters

        def final():
            eng.anticipated_paths(B, C, T, R, hold["eps2"], x0=x0, out=o_x)

        def composed():
            mz_paths()
            unconstrained()
            regime_loop()
            final()

        setup = lambda: eng.anticipated_paths(B, C, T, R, eps, outputs=("G",), out=g_only)  # noqa: E731
        entry()
        composed()
        torch.cuda.synchronize()
        it = eng.constrained_paths(B, C, T, R, eps, c, bound, shock, H, x0=x0, outputs=("iters", "path_status"))
        torch.cuda.synchronize()
        ok = (it["path_status"] & (_lib.OBC_NO_REGIME | _lib.OBC_SINGULAR | _lib.OBC_SKIPPED)) == 0  # (the others are NaN by the entry)
        diff = (out["x"][ok] - o_x["x"][ok]).abs().max().item() / o_x["x"][ok].abs().max().item()
        assert diff <= 1e-9, diff
        print(f"draws={nb:5d} paths without a regime: {int((~ok).sum())} of {ok.numel()}; status words seen {sorted(set(it['status'].tolist()))}")
        print(f"draws={nb:5d} entry against the composed route: {diff:.1e} of max|x|; iters mean {it['iters'].double().mean().item():.2f} max "
              f"{int(it['iters'].max())} (composed loop: {hold['iters']} round trips); path_status bits seen {sorted(set(it['path_status'].flatten().tolist()))}")
        t_entry, t_comp, t_nu = med(entry), med(composed), med(to_nu)
        t_setup, t_mz, t_xu, t_loop, t_final = med(setup), med(mz_paths), med(unconstrained), med(regime_loop), med(final)
        print(f"draws={nb:5d} entry {t_entry:8.3f} ms | composed route {t_comp:8.3f} ms = Mz paths {t_mz:8.3f} + unconstrained {t_xu:8.3f} + torch "
              f"regime loop {t_loop:8.3f} + final paths {t_final:8.3f} (sum {t_mz + t_xu + t_loop + t_final:8.3f}) | entry / composed {t_entry / t_comp:5.2f}")
        print(f"draws={nb:5d} phase split of the entry: setup {t_setup:8.3f} ms, Mz paths {t_mz - t_setup:8.3f}, unconstrained paths (H periods) "
              f"{t_xu - t_setup:8.3f}, regime + gap kernels (outputs=('nu',) less the three before) {t_nu - t_mz - t_xu + t_setup:8.3f}, final paths "
              f"and the gap over them (entry less outputs=('nu',)) {t_entry - t_nu:8.3f}")


def stochastic_bound_rows(eng, sizes, n_steps=N_STEPS, n_paths=16, horizon=32, shock=0, repeats=5):
    """The workload of --constrained with fresh (surprise) shocks every period: LogpEngine.constrained_simulate against the composed
    route of the public calls before it -- Mz and G once from constrained_paths(outputs=("Mz",)) and anticipated_paths(outputs=("G",)),
    the tables Cq and W by torch products, then per period bmm for xu and q, the torch regime loop of --constrained, and the update."""
    b = wl.sw_shaped_batch(64)
    m, k, H = 40, 7, horizon
    rng = np.random.default_rng(0)
    D64 = rng.standard_normal((64, m, k)) / np.sqrt(m)
    R64 = np.stack([np.linalg.solve(b["B"][i] + b["C"][i] @ b["T_star"][i], -D64[i]) for i in range(64)])
    var = np.argmax(np.abs(R64[:, :, shock]), axis=1)
    c64 = np.zeros((64, m))
    c64[np.arange(64), var] = np.sign(R64[np.arange(64), var, shock])
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    print(f"stochastic simulation at the bound m={m} k={k}, dense impact matrix, {n_steps} steps, {n_paths} paths, surprise shocks at every "
          f"step, H={H}, bound at half the unconstrained simulated minimum; medians of {repeats} timings of >= 1 s")
    for nb in sizes:
        rep = (nb + 63) // 64
        B, C, T, R = (eng.to_device(np.tile(a, (rep, 1, 1))[:nb]) for a in (b["B"], b["C"], b["T_star"], R64))
        c = eng.to_device(np.tile(c64, (rep, 1))[:nb])
        eps = eng.to_device(rng.standard_normal((nb, n_paths, n_steps, k)) * 0.01)
        x0 = eng.to_device(rng.standard_normal((nb, n_paths, m)) * 0.05)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        cx, x = [], x0  # the unconstrained simulation, for the bound
        for t in range(n_steps):
            x = torch.baddbmm(torch.bmm(eps[:, :, t], R.transpose(1, 2)), x, T.transpose(1, 2))
            cx.append(torch.einsum("bpn,bn->bp", x, c))
        bound = (0.5 * torch.stack(cx, dim=-1).amin(dim=(1, 2))).contiguous()
        out, out_mz = dict(x=mk(nb, n_paths, n_steps, m)), dict(Mz=mk(nb, H, H))
        entry = lambda: eng.constrained_simulate(B, C, T, R, eps, c, bound, shock, H, x0=x0, out=out)  # noqa: E731
        to_mz = lambda: eng.constrained_simulate(B, C, T, R, eps, c, bound, shock, H, x0=x0, outputs=("Mz",), out=out_mz)  # noqa: E731
        # the composed route
        eye = torch.eye(H, dtype=torch.float64, device=eng.device)
        o_mz, g_only, x_c = dict(Mz=mk(nb, H, H)), dict(G=mk(nb, m, m)), mk(nb, n_paths, n_steps, m)
        hold, e1 = dict(iters=0), eps[:, :1, :1].contiguous()  # (Mz and G do not depend on the shocks)

        def tables():
            eng.constrained_paths(B, C, T, R, e1, c, bound, shock, H, n_steps=H, outputs=("Mz",), out=o_mz)
            eng.anticipated_paths(B, C, T, R, e1, outputs=("G",), out=g_only)
            rows, cols = [c[:, None, :]], [R[:, :, shock:shock + 1]]
            for _ in range(H - 1):
                rows.append(torch.bmm(rows[-1], T))
                cols.append(torch.bmm(g_only["G"], cols[-1]))
            hold["Cq"], hold["W"] = torch.cat(rows, dim=1), torch.cat(cols, dim=2)  # (nb, H, m), (nb, m, H)

        def periods():
            Mz, Cq, W = o_mz["Mz"], hold["Cq"], hold["W"]
            x = x0
            alive = torch.ones(nb, n_paths, dtype=torch.bool, device=eng.device)
            for t in range(n_steps):
                xu_t = torch.baddbmm(torch.bmm(eps[:, :, t], R.transpose(1, 2)), x, T.transpose(1, 2))  # (nb, n_paths, m)
                q = torch.bmm(xu_t, Cq.transpose(1, 2)) - bound[:, None, None]
                S, iters = q < 0.0, 0
                while True:
                    iters += 1
                    d = S.to(torch.float64)
                    K = eye + d[..., :, None] * (Mz[:, None] - eye) * d[..., None, :]
                    nu = torch.linalg.solve(K, (-q * d)[..., None])[..., 0]
                    gap = q + torch.einsum("bhj,bpj->bph", Mz, nu)
                    S_new = torch.where(S, nu > 0.0, gap < 0.0)
                    same = (S_new == S).all(dim=-1)
                    if bool(same.all()) or iters >= 64:  # (the host round trip of every iteration)
                        break
                    S = torch.where(same[..., None], S, S_new)  # a path that has its regime keeps it
                alive = alive & same
                hold["iters"] = max(hold["iters"], iters)
                x = xu_t + torch.bmm(nu, W.transpose(1, 2))
                x_c[:, :, t] = x
            hold["alive"] = alive

        entry()
        tables()
        periods()
        torch.cuda.synchronize()
        it = eng.constrained_simulate(B, C, T, R, eps, c, bound, shock, H, x0=x0, outputs=("iters", "duration", "path_status", "fail_step"))
        torch.cuda.synchronize()
        ok = ((it["path_status"] & (_lib.OBC_NO_REGIME | _lib.OBC_SINGULAR | _lib.OBC_SKIPPED)) == 0) & hold["alive"]
        diff = (out["x"][ok] - x_c[ok]).abs().max().item() / x_c[ok].abs().max().item()
        good = it["fail_step"] < 0
        print(f"draws={nb:5d} failed paths: {int((~good).sum())} of {good.numel()} (composed route: {int((~hold['alive']).sum())} without a regime "
              f"in some period); path_status bits seen {sorted(set(it['path_status'].flatten().tolist()))}; status words seen "
              f"{sorted(set(it['status'].tolist()))}")
        print(f"draws={nb:5d} entry against the composed route on the paths both resolve: {diff:.1e} of max|x|; iters mean "
              f"{it['iters'][good].double().mean().item():.2f} max {int(it['iters'].max())}, duration mean "
              f"{it['duration'][good].double().mean().item():.2f} max {int(it['duration'].max())} (composed loop: up to {hold['iters']} round "
              f"trips in a period)")
        assert diff <= 1e-9, diff
        t_entry, t_mz, t_tab = med(entry), med(to_mz), med(tables)
        # (the period loop has run once above; a call of it takes seconds where paths without a regime hold it for 64 round trips)
        t_per = float(np.median([timed(periods, warm=0, calls=1) for _ in range(repeats)]))
        t_comp = t_tab + t_per
        print(f"draws={nb:5d} entry {t_entry:8.3f} ms | composed route {t_comp:8.3f} ms = Mz, G and tables {t_tab:8.3f} + {n_steps} periods "
              f"{t_per:8.3f} | entry / composed {t_entry / t_comp:5.2f}")
        print(f"draws={nb:5d} phase split of the entry: outputs=('Mz',) (Mz chain, tables, a simulation that writes only Mz) {t_mz:8.3f} ms, "
              f"entry less that {t_entry - t_mz:8.3f} ms")


def segmented_rows(eng, sizes, T_len=200, repeats=5):
    """The Kalman likelihood across dated breaks (csrc/dsge_kalman_seg.hpp) on the SW-shaped batch (n = 40, T_len = 200, p and Z of
    bench.py's workload): S = 1, S = 3 with breaks at 80 and 140, S = 8, against the full recursions a caller had before it --
    dsge_kalman_filter_outputs_batched with ll alone, and for scale dsge_kalman_logp_batched with kalman_steady_tol = 0 and at its
    default.  Segment s of draw b is draw (b + s) mod 64 of the generator."""
    lib = _lib.load()
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p = 40, 7, om["y"].shape[1]
    y, H1, Z1 = eng.to_device(om["y"][:T_len]), om["Hdiag"], om["Z"]
    breaks = {1: (0,), 3: (0, 80, 140), 8: tuple(range(0, T_len, T_len // 8))[:8]}
    ns, zs = int(np.count_nonzero(np.any(b["T_star"] != 0, axis=(0, 1)))), 1
    print(f"segmented filter, SW shape m={m} k={k} p={p}, T_len={T_len}; median of {repeats} timings of >= 1 s each")
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    for nb in sizes:
        idx = np.arange(nb) % 64
        T, R, q = eng.to_device(b["T_star"][idx]), eng.to_device(R64[idx]), eng.to_device(b["sigma"][idx] ** 2)
        Z, H = eng.to_device(Z1), eng.to_device(H1)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        ll, logp = mk(nb, T_len), mk(nb)
        st = torch.zeros(nb, dtype=torch.int32, device=eng.device)

        def filter_outputs():
            _lib.check(lib.dsge_kalman_filter_outputs_batched(
                T.data_ptr(), R.data_ptr(), q.data_ptr(), 1, Z.data_ptr(), 0, None, 0, H.data_ptr(), 0, y.data_ptr(), nb, m, k, p,
                T_len, 1e-8, -9999.0, ll.data_ptr(), None, None, None, None, 0, st.data_ptr(), eng._stream()))

        def fast(options):
            with _lib.options_scope(options):
                _lib.check(lib.dsge_kalman_logp_batched(
                    T.data_ptr(), R.data_ptr(), q.data_ptr(), 1, Z.data_ptr(), 0, None, 0, H.data_ptr(), 0, y.data_ptr(), nb, m, k, p,
                    T_len, 1e-8, -9999.0, ns, zs, logp.data_ptr(), st.data_ptr(), eng._stream()))

        t_ko = med(filter_outputs)
        ll_ko = ll.clone()
        no_steady = _lib.make_options(kalman_steady_tol=0.0)
        t_full, t_fast = med(lambda: fast(no_steady)), med(lambda: fast(None))
        assert int(st.abs().max().item()) == 0
        print(f"draws={nb:5d} filter outputs, ll alone: {t_ko:9.3f} ms | kalman_logp, no steady state: {t_full:8.3f} ms | "
              f"kalman_logp, default: {t_fast:8.3f} ms")
        t_one = None
        for S, starts in breaks.items():
            pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % 64
            Ts, Rs, qs = eng.to_device(b["T_star"][pick]), eng.to_device(R64[pick]), eng.to_device(b["sigma"][pick] ** 2)
            Zs, Hs = eng.to_device(np.tile(Z1, (S, 1, 1))), eng.to_device(np.tile(H1, (S, 1)))
            out = dict(logp=logp)
            call = lambda outputs, out: eng.kalman_logp_segments(Ts, Rs, qs, Zs, y, starts, Hdiag=Hs, q_mode="diag_batched",  # noqa: E731
                                                                  outputs=outputs, out=out, status=st)
            t_lp = med(lambda: call(("logp",), out))
            t_ll = med(lambda: call(("logp", "ll"), dict(logp=logp, ll=ll)))
            assert int(st.abs().max().item()) == 0
            if S == 1:
                t_one = t_lp
                agree = float((ll - ll_ko).abs().max() / ll_ko.abs().max())
                print(f"draws={nb:5d} S=1 against the filter outputs, largest |ll difference| / max |ll|: {agree:.2e}")
            print(f"draws={nb:5d} segments S={S} breaks {starts if S < 8 else 'every ' + str(T_len // 8)}: logp alone {t_lp:9.3f} ms, "
                  f"with ll {t_ll:9.3f} ms | / S=1: {t_lp / t_one:5.3f} | / filter outputs: {t_lp / t_ko:5.3f} | "
                  f"/ kalman_logp no steady: {t_lp / t_full:6.2f} | / default: {t_lp / t_fast:6.2f}")


def segmented_smoother_rows(eng, sizes, other_lib=None, scratch_limit=0, T_len=200, repeats=5):
    """The smoother across dated breaks (docs/design/segmented_smoother.md) on the SW-shaped batch of ``segmented_rows``: S = 1,
    S = 3 with breaks at 80 and 140, S = 8, with diagonal covariances and without covariances (ll, states and shocks in both),
    against dsge_kalman_smoother_batched on the inputs of S = 1 -- of this build and, with ``--library PATH``, of the libdsge_hip.so
    at PATH (a build of the parent commit) loaded next to it.  ``scratch_limit`` (``--scratch-limit-gib``; 0: the library's 2 GiB)
    is the ``scratch_limit_bytes`` of every call: the stored forward pass takes 5.3 MB per draw at this shape, so by default the
    batch goes in chunks of about 400 draws (fewer with more segments: their bases count too)."""
    import ctypes

    libs = {"this build": _lib.load()}
    if other_lib:
        libs[other_lib] = ctypes.CDLL(other_lib)
        libs[other_lib].dsge_kalman_smoother_batched.argtypes = _lib.PROTOTYPES["dsge_kalman_smoother_batched"]
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p = 40, 7, om["y"].shape[1]
    y, H1, Z1 = eng.to_device(om["y"][:T_len]), om["Hdiag"], om["Z"]
    breaks = {1: (0,), 3: (0, 80, 140), 8: tuple(range(0, T_len, T_len // 8))[:8]}
    print(f"segmented smoother, SW shape m={m} k={k} p={p}, T_len={T_len}, scratch_limit_bytes={scratch_limit}; median of {repeats} "
          "timings of >= 1 s each")
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    for nb in sizes:
        idx = np.arange(nb) % 64
        T, R, q = eng.to_device(b["T_star"][idx]), eng.to_device(R64[idx]), eng.to_device(b["sigma"][idx] ** 2)
        Z, H = eng.to_device(Z1), eng.to_device(H1)
        mk = lambda *sh: torch.empty(sh, dtype=torch.float64, device=eng.device)  # noqa: E731
        ll, a_s, p_s, e_s = mk(nb, T_len), mk(nb, T_len, m), mk(nb, T_len, m), mk(nb, T_len, k)
        st = torch.zeros(nb, dtype=torch.int32, device=eng.device)
        plain, kept = {}, {}
        for name, lib in libs.items():
            def smoother(cov, lib=lib):
                _lib.check(lib.dsge_kalman_smoother_batched(
                    T.data_ptr(), R.data_ptr(), q.data_ptr(), 1, Z.data_ptr(), 0, None, 0, H.data_ptr(), 0, y.data_ptr(), nb, m, k, p,
                    T_len, 1e-8, -9999.0, 0.0, scratch_limit, ll.data_ptr(), a_s.data_ptr(), p_s.data_ptr() if cov else None, e_s.data_ptr(), 0,
                    st.data_ptr(), eng._stream()))

            plain[name] = (med(lambda: smoother(True)), med(lambda: smoother(False)))
            smoother(True)
            kept[name] = [x.clone() for x in (ll, a_s, p_s, e_s)]
            assert int(st.abs().max().item()) == 0
            print(f"draws={nb:5d} kalman_smoother_batched of {name}: diagonal covariances {plain[name][0]:9.3f} ms, "
                  f"no covariances {plain[name][1]:9.3f} ms")
        base = plain[other_lib] if other_lib else plain["this build"]
        one = None
        for S, starts in breaks.items():
            pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % 64
            Ts, Rs, qs = eng.to_device(b["T_star"][pick]), eng.to_device(R64[pick]), eng.to_device(b["sigma"][pick] ** 2)
            Zs, Hs = eng.to_device(np.tile(Z1, (S, 1, 1))), eng.to_device(np.tile(H1, (S, 1)))
            out = dict(ll=ll, smoothed_states=a_s, smoothed_covs=p_s, smoothed_shocks=e_s)
            lean = {key: v for key, v in out.items() if key != "smoothed_covs"}
            call = lambda out: eng.kalman_smoother_segments(Ts, Rs, qs, Zs, y, starts, Hdiag=Hs, q_mode="diag_batched",  # noqa: E731
                                                            outputs=tuple(out), out=out, status=st,
                                                            scratch_limit_bytes=scratch_limit)
            t = (med(lambda: call(out)), med(lambda: call(lean)))
            assert int(st.abs().max().item()) == 0
            if S == 1:
                one = t
                call(out)
                for name, ref in kept.items():
                    same = [bool(torch.equal(torch.nan_to_num(x), torch.nan_to_num(r))) for x, r in zip((ll, a_s, p_s, e_s), ref)]
                    print(f"draws={nb:5d} S=1 against kalman_smoother_batched of {name}, bit-identical (ll, states, covs, shocks): {same}")
            print(f"draws={nb:5d} segments S={S} breaks {starts if S < 8 else 'every ' + str(T_len // 8)}: diagonal covariances "
                  f"{t[0]:9.3f} ms, no covariances {t[1]:9.3f} ms | / S=1: {t[0] / one[0]:5.3f}, {t[1] / one[1]:5.3f} | "
                  f"/ kalman_smoother_batched: {t[0] / base[0]:5.3f}, {t[1] / base[1]:5.3f} | per boundary: "
                  f"{(t[0] - one[0]) / max(S - 1, 1) * 1e3:8.1f} us, {(t[1] - one[1]) / max(S - 1, 1) * 1e3:8.1f} us")


def segmented_gradient_rows(eng, sizes, other_lib=None, scratch_limit=0, T_len=200, repeats=5):
    """The gradient of the likelihood across dated breaks (docs/design/segmented_gradient.md) on the SW-shaped batch of
    ``segmented_rows``: every cotangent, S = 1, S = 3 with breaks at 80 and 140, S = 8, next to dsge_kalman_logp_segments_batched
    (logp alone) of the library at ``--library PATH`` (a build of the parent commit; this build's without it) on the same inputs."""
    import ctypes

    name = "dsge_kalman_logp_segments_batched"
    lib = _lib.load()
    if other_lib:
        lib = ctypes.CDLL(other_lib)
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p = 40, 7, om["y"].shape[1]
    y, H1, Z1 = eng.to_device(om["y"][:T_len]), om["Hdiag"], om["Z"]
    breaks = {1: (0,), 3: (0, 80, 140), 8: tuple(range(0, T_len, T_len // 8))[:8]}
    print(f"segmented gradient, SW shape m={m} k={k} p={p}, T_len={T_len}, scratch_limit_bytes={scratch_limit}; median of {repeats} "
          f"timings of >= 1 s each; likelihood: {name} of {other_lib or 'this build'}")
    med = lambda fn: float(np.median([timed(fn) for _ in range(repeats)]))  # noqa: E731
    for nb in sizes:
        for S, starts in breaks.items():
            pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % 64
            Ts, Rs, qs = eng.to_device(b["T_star"][pick]), eng.to_device(R64[pick]), eng.to_device(b["sigma"][pick] ** 2)
            Zs, Hs = eng.to_device(np.tile(Z1, (S, 1, 1))), eng.to_device(np.tile(H1, (S, 1)))
            seg = np.ascontiguousarray(starts, dtype=np.int32)
            logp = torch.empty(nb, dtype=torch.float64, device=eng.device)
            st = torch.zeros(nb, dtype=torch.int32, device=eng.device)

            def likelihood():
                _lib.check(getattr(lib, name)(
                    Ts.data_ptr(), Rs.data_ptr(), qs.data_ptr(), 1, Zs.data_ptr(), 0, None, 0, Hs.data_ptr(), 0, None, None, None,
                    y.data_ptr(), seg.ctypes.data, S, nb, m, k, p, T_len, 1e-8, -9999.0, logp.data_ptr(), None, None, None, st.data_ptr(),
                    eng._stream()))

            t_lp = med(likelihood)
            likelihood()
            lp_kept = logp.clone()
            out = {}

            def gradient():
                out.update(eng.kalman_logp_segments_grad(Ts, Rs, qs, Zs, y, starts, Hdiag=Hs, q_mode="diag_batched", status=st,
                                                         scratch_limit_bytes=scratch_limit, out={key: v for key, v in out.items()
                                                                                                  if key != "status"}))

            t_g = med(gradient)
            assert int(st.abs().max().item()) == 0
            same = bool(torch.equal(out["logp"], lp_kept))
            n_fd = 2 * m * m
            print(f"draws={nb:5d} segments S={S} breaks {starts if S < 8 else 'every ' + str(T_len // 8)}: likelihood {t_lp:9.3f} ms | "
                  f"gradient, every cotangent {t_g:9.3f} ms | gradient / likelihood {t_g / t_lp:6.2f} | logp bit-identical: {same} | "
                  f"one T_s alone by central differences: {n_fd} likelihood calls = {n_fd * t_lp * 1e-3:9.1f} s (stated, not run)")


def main():
    other_lib, scratch_limit = None, 0
    for flag in ("--library", "--scratch-limit-gib"):
        if flag in sys.argv:
            at = sys.argv.index(flag)
            if flag == "--library":
                other_lib = sys.argv[at + 1]
            else:
                scratch_limit = int(float(sys.argv[at + 1]) * 2 ** 30)
            del sys.argv[at:at + 2]
    args = [a for a in sys.argv[1:] if a not in ("--second-order", "--decomposition", "--conditional", "--spectral", "--anticipated",
                                                 "--constrained", "--stochastic-bound", "--segmented", "--segmented-smoother",
                                                 "--segmented-gradient")]
    sizes = [int(a) for a in args] or [256, 4096]
    if "--segmented-gradient" in sys.argv:
        return segmented_gradient_rows(LogpEngine(0), sizes, other_lib, scratch_limit)
    if "--segmented-smoother" in sys.argv:
        return segmented_smoother_rows(LogpEngine(0), sizes, other_lib, scratch_limit)
    if "--second-order" in sys.argv:
        return second_order_rows(LogpEngine(0), sizes)
    if "--decomposition" in sys.argv:
        return decomposition_rows(LogpEngine(0), sizes)
    if "--conditional" in sys.argv:
        return conditional_rows(LogpEngine(0), sizes)
    if "--spectral" in sys.argv:
        return spectral_rows(LogpEngine(0), sizes)
    if "--anticipated" in sys.argv:
        return anticipated_rows(LogpEngine(0), sizes)
    if "--constrained" in sys.argv:
        return constrained_rows(LogpEngine(0), sizes)
    if "--stochastic-bound" in sys.argv:
        return stochastic_bound_rows(LogpEngine(0), sizes)
    if "--segmented" in sys.argv:
        return segmented_rows(LogpEngine(0), sizes)
    eng = LogpEngine(0)
    lib = _lib.load()
    b = wl.sw_shaped_batch(64)
    om = wl.sw_shaped_observation_model()
    R64 = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], b["T_star"][i]) for i in range(64)])
    m, k, p = 40, 7, om["y"].shape[1]
    Z, y, H = eng.to_device(om["Z"]), eng.to_device(om["y"][:N_STEPS]), eng.to_device(om["Hdiag"])
    rng = np.random.default_rng(0)
    print(f"SW shape m={m} k={k}, {N_STEPS} steps")
    for nb in sizes:
        rep = (nb + 63) // 64
        Th, Rh, qh = np.tile(b["T_star"], (rep, 1, 1))[:nb], np.tile(R64, (rep, 1, 1))[:nb], np.tile(b["sigma"] ** 2, (rep, 1))[:nb]
        T, R, q = eng.to_device(Th), eng.to_device(Rh), eng.to_device(qh)
        mk = lambda *s: torch.empty(s, dtype=torch.float64, device=eng.device)  # noqa: E731
        irf, fevd, paths = mk(nb, k, N_STEPS, m), mk(nb, N_STEPS, m, k), mk(nb, 16, N_STEPS, m)
        eps = eng.to_device(rng.standard_normal((nb, 16, N_STEPS, k)))
        a0, P0 = eng.to_device(rng.normal(0, 0.01, (nb, m))), eng.to_device(np.tile(1e-4 * np.eye(m), (nb, 1, 1)))
        fc = dict(states=mk(nb, N_STEPS, m), covs=mk(nb, N_STEPS, m, m))
        ll, ap, af, pp, pf = mk(nb, N_STEPS), mk(nb, N_STEPS, m), mk(nb, N_STEPS, m), mk(nb, N_STEPS, m, m), mk(nb, N_STEPS, m, m)
        st = torch.zeros(nb, dtype=torch.int32, device=eng.device)

        def filter_outputs():
            _lib.check(lib.dsge_kalman_filter_outputs_batched(
                T.data_ptr(), R.data_ptr(), q.data_ptr(), 1, Z.data_ptr(), 0, None, 0, H.data_ptr(), 0, y.data_ptr(), nb, m, k, p,
                N_STEPS, 1e-8, -9999.0, ll.data_ptr(), ap.data_ptr(), af.data_ptr(), pp.data_ptr(), pf.data_ptr(), 1, st.data_ptr(),
                eng._stream()))

        t_irf = timed(lambda: eng.impulse_response(T, R, n_steps=N_STEPS, out=dict(irf=irf)))
        t_irf_fill = timed(lambda: irf.fill_(1.0))
        t_fevd = timed(lambda: eng.impulse_response(T, R, n_steps=N_STEPS, weights=q, fevd=True, out=dict(irf=irf, fevd=fevd)))
        t_sim = timed(lambda: eng.simulate(T, R, eps, out=paths))
        t_sim_fill = timed(lambda: paths.fill_(1.0))
        t_fc = timed(lambda: eng.forecast(T, R, q, a0, P0, n_steps=N_STEPS, covariances="full", q_mode=1, out=fc))
        t_ko = timed(filter_outputs)
        assert int(st.abs().max().item()) == 0
        for name, t, tf, out in (("impulse responses", t_irf, t_irf_fill, irf), ("simulate, 16 paths", t_sim, t_sim_fill, paths)):
            gb = out.numel() * 8e-9
            print(f"draws={nb:5d} {name:20s}: {t:8.3f} ms = {gb / t:6.2f} TB/s written | fill {tf:8.3f} ms = {gb / tf:6.2f} TB/s | "
                  f"ratio {t / tf:5.2f}")
        print(f"draws={nb:5d} impulse responses + FEVD: {t_fevd:8.3f} ms")
        print(f"draws={nb:5d} forecast, full covs : {t_fc:8.3f} ms | filter outputs, full covs, T_len={N_STEPS}: {t_ko:8.3f} ms | "
              f"ratio {t_fc / t_ko:5.2f}")
        nc = min(nb, 256)  # host numpy loop over (a sample of) the draws, scaled to the batch
        t0 = time.perf_counter()
        for i in range(nc):
            dr.impulse_responses(Th[i], Rh[i], N_STEPS)
        t_cpu_irf = (time.perf_counter() - t0) / nc * nb * 1e3
        t0 = time.perf_counter()
        for i in range(nc):
            dr.forecast(Th[i], Rh[i], qh[i], np.zeros(m), 1e-4 * np.eye(m), N_STEPS)
        t_cpu_fc = (time.perf_counter() - t0) / nc * nb * 1e3
        print(f"draws={nb:5d} host numpy loop ({nc} draws timed, scaled): impulse responses {t_cpu_irf:9.1f} ms ({t_cpu_irf / t_irf:7.0f}x), "
              f"forecast {t_cpu_fc:9.1f} ms ({t_cpu_fc / t_fc:7.0f}x)")
    second_order_rows(eng, sizes)


if __name__ == "__main__":
    main()
