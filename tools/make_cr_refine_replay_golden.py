"""GPU box: record what the cycle-reduction kernels return on systems that take the refinement branch of crc_iterate
(csrc/dsge_cr_compact.hpp), bit for bit, into tests/golden/cr_refine_replay_parent.npz.

    python tools/make_cr_refine_replay_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned: the PARENT of the change that refines by replaying the recorded
elimination instead of eliminating [A1 | R - A1 X] a second time (docs/design/cycle_reduction.md 4.1j).  The test
tests/test_gpu_cr_refine_replay.py then compares a later build with np.array_equal.  Batches of at most 16 systems.

A system refines because ONE equation is scaled by 1e-5 (as tests/test_gpu_cr_rhs_registers.py does it): the scaling survives
every update of A1, so such a draw refines in EVERY iteration.  host_pivot_ratios replays the iteration and the pivots in numpy;
the test asserts from it that every case is a factor ten beyond its tile's rule.

    compact_n<N>        cycle_reduction_batched (cr_compact_kernel<BS>, BS = ceil(N / 8)): per tile the smallest n, an n with a
                        partial last panel, n equal to the tile; four systems each, all refine in every iteration.  49 .. 64
                        variables run with cr_four_waves = 0 (the default there is the four-wavefront kernel, not this branch)
    compact_one_wave    n = 30 with cr_two_waves = 0 (cr_compact_kernel<4> next to the default cr_compact_kernel_occ2<4>)
    late_n40            SW-shaped bench draws (40 variables, the (5)-wide tile): draws that do not refine in the first iteration and
                        do later, next to draws that never do (LATE_DRAWS: found with host_pivot_ratios).  cr_compact_kernel<5>, an
                        instance that eliminates twice: the pin of the non-replaying code
    late_fused_n40      the same draws with D, sigma and the bench's observation model (12 periods) through the fused likelihood call
                        with the static hint 10: cr_fused_kernel_occ2<5, 4>, the bench's own path, which replays -- iterations that
                        skip the branch in front of iterations that replay, each its own record; late on the REDUCED system too
    late_n30            30 variables through cycle_reduction_batched, cr_compact_kernel_occ2<4> (replays): a system that refines in
                        its fourth and fifth iteration only (LATE30_SEEDS[0], found by the same search) next to two that never do
    mixed_n30           one batch: refining, plain, not converging (T^2 + T / 2 + 1 = 0 times M: roots on the unit circle), NaN,
                        refining
    scan_n30            scan_cycle_reduction_batched on refining systems
    fused_n20, _n40     the one-launch deflated kernel through the fused likelihood call with T and R returned: instances (3, 2) and
                        (5, 4); the scaled equation has zeros in the static columns, so the reflectors leave it alone
    fused_n32, _n42     its other instances with the register budget of two waves per SIMD, the ones that replay: (4, 4) with 7 of 8
                        static variables deflated, (6, 4) with 10 of 12
    fused_n56           a wide instance with three columns per lane, (7, 6, 3): 8 of 14 static variables (it eliminates twice)
    three_launch_n12    12 variables, 3 static: cr_deflate -> cr_compact -> cr_inflate
    logp_n40            fused_n40 without T and R: logp and status
"""
from __future__ import annotations

import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "cr_refine_replay_parent.npz")
TOL, MAX_ITER = 1e-9, 1000
SCALE = 1e-5
COMPACT_N = (2, 8, 9, 13, 16, 17, 22, 24, 25, 30, 32, 33, 38, 40, 41, 46, 48, 49, 53, 56, 57, 61, 64)
# bench draws: 964 and 1781 stay below the rule in the first iteration and pass ten times the rule in the third / second (964 in
# two iterations), 752 refines in every iteration, 0 and 1 never (host_pivot_ratios; `late` on the command line searches)
LATE_DRAWS = (964, 1781, 752, 0, 1)
LATE_REFINING = (0, 1)  # positions in LATE_DRAWS
LATE30_SEED0, LATE30_SEEDS, LATE30_SHAPE = 1717000, (1562, 0, 1), dict(n=30, n_state=14, n_lead=10, k=5)  # (the first one refines late)
# name -> (n, n_state, n_lead, k, static hint, draws, p, T_len)
FUSED = {"fused_n20": (20, 9, 7, 3, 4, 4, 3, 12), "fused_n40": (40, 18, 12, 7, 10, 4, 7, 12), "three_launch_n12": (12, 5, 4, 3, 3, 4, 3, 12),
         "logp_n40": (40, 18, 12, 7, 10, 4, 7, 12), "fused_n32": (32, 14, 10, 5, 7, 4, 5, 12), "fused_n42": (42, 18, 12, 7, 10, 4, 7, 12),
         "fused_n56": (56, 24, 18, 7, 8, 4, 7, 12), "late_fused_n40": (40, 18, 12, 7, 10, len(LATE_DRAWS), 7, 12)}
CASES = tuple("compact_n%d" % n for n in COMPACT_N) + ("compact_one_wave", "late_n40", "late_n30", "mixed_n30", "scan_n30") + tuple(FUSED)


def bs_of(n):
    return max(1, (n + 7) // 8)


def refine_rule(n):
    """cr_refine_ratio<BS>() of csrc/dsge_device.hpp."""
    bs = bs_of(n)
    return 1e3 if (bs <= 3 or bs > 5) else 3e3


def _rescale(M, target):
    return M * (target / np.max(np.abs(np.linalg.eigvals(M))))


def reversal_system(seed, n, scaled=True):
    """A + B T* + C T*^2 = 0 with M = P + 0.05 noise, P the reversal permutation (column c pivots on row n - 1 - c), rho(T*[S,S])
    = 0.6, rho(G) = 0.3: six or seven iterations.  scaled: the equation that pivots the LAST column times SCALE."""
    ns, nl = max(1, n // 2), max(1, n // 3)
    rng = np.random.default_rng([17100 + seed, n])
    T_star = np.zeros((n, n))
    T_star[:ns, :ns] = _rescale(rng.standard_normal((ns, ns)), 0.6)
    T_star[ns:, :ns] = 0.3 * rng.standard_normal((n - ns, ns))
    G = np.zeros((n, n))
    G[:, n - nl:] = rng.standard_normal((n, nl))
    G = _rescale(G, 0.3)
    M = np.eye(n)[::-1] + 0.05 * rng.standard_normal((n, n))
    C = M @ G
    B = M - C @ T_star
    A = -M @ T_star
    if scaled:
        for X in (A, B, C):
            X[0] *= SCALE
    return A, B, C


def deflatable_system(seed, n, ns, nl, k):
    """workloads.sw_shaped_system with the LAST equation free of the static variables ns .. n - nl - 1 and scaled by SCALE."""
    rng = np.random.default_rng(seed)
    S = _rescale(rng.standard_normal((ns, ns)), 0.95 * rng.uniform(0.5, 1.0))
    T_star = np.zeros((n, n))
    T_star[:ns, :ns] = S
    T_star[ns:, :ns] = 0.3 * rng.standard_normal((n - ns, ns))
    G = np.zeros((n, n))
    G[:, n - nl:] = rng.standard_normal((n, nl))
    G = _rescale(G, rng.uniform(0.3, 0.8))
    M = np.eye(n) + 0.2 * rng.standard_normal((n, n))
    M[n - 1, ns:n - nl] = 0.0
    C = M @ G
    B = M - C @ T_star
    A = -M @ T_star
    E = np.zeros((n, k))
    E[:k, :k] = -np.eye(k)
    D = M @ E
    for X in (A, B, C, D):
        X[n - 1] *= SCALE
    return A, B, C, D


def pivot_ratio(A1):
    """Largest over smallest |pivot| of Gauss-Jordan with partial pivoting among the rows not yet used (the device's order)."""
    W = np.array(A1, dtype=np.float64)
    n = W.shape[0]
    free = np.ones(n, dtype=bool)
    piv = []
    for c in range(n):
        r = int(np.argmax(np.where(free, np.abs(W[:, c]), -1.0)))
        free[r] = False
        piv.append(abs(W[r, c]))
        f = W[:, c] / W[r, c]
        f[r] = 0.0
        W -= np.outer(f, W[r])
    return max(piv) / min(piv)


def host_pivot_ratios(A, B, C, tol=TOL, max_iter=60):
    """The pivot ratio of A1 in every iteration of the cycle reduction (numpy replay of crc_iterate's recurrences)."""
    A0, A1, A2 = (np.array(X, dtype=np.float64) for X in (A, B, C))
    out = []
    for _ in range(max_iter):
        out.append(pivot_ratio(A1))
        X0, X2 = np.linalg.solve(A1, A0), np.linalg.solve(A1, A2)
        A1 = A1 - A0 @ X2 - A2 @ X0
        A0, A2 = -A0 @ X0, -A2 @ X2
        if np.abs(A0).sum(axis=0).max() < tol and np.abs(A2).sum(axis=0).max() < tol:
            break
    return np.array(out)


def reduced_system(A, B, C, h):
    """The system the deflated kernels iterate on: the first h static columns of B triangularised by Householder reflectors, their
    rows and columns dropped.  (An equation with zeros in those columns is left alone by every reflector.)"""
    n = A.shape[0]
    static = np.flatnonzero(~((A != 0).any(axis=0) | (C != 0).any(axis=0)))[:h]
    dyn = np.setdiff1d(np.arange(n), static)
    Q, _ = np.linalg.qr(B[:, static], mode="complete")
    return tuple((Q.T @ X)[h:][:, dyn] for X in (A, B, C))


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of read-only arrays (A, B, C and, for the fused cases, D, sig, Z, y, Hdiag) and `refines`: per draw, whether it is
    built to refine (None: not by scaling, see late_n40)."""
    from geconpy_amd import workloads as wl

    out = {}
    if name.startswith("compact_n") or name in ("compact_one_wave", "scan_n30"):
        n = int(name[9:]) if name.startswith("compact_n") else 30
        sys_ = [reversal_system(seed, n) for seed in range(4)]
        out = dict(A=np.stack([s[0] for s in sys_]), B=np.stack([s[1] for s in sys_]), C=np.stack([s[2] for s in sys_]))
        refines = [True] * 4
    elif name == "late_n40":
        b = wl.sw_shaped_batch(max(LATE_DRAWS) + 1)
        idx = list(LATE_DRAWS)
        out = dict(A=b["A"][idx].copy(), B=b["B"][idx].copy(), C=b["C"][idx].copy())
        refines = None
    elif name == "late_fused_n40":
        b = wl.sw_shaped_batch(max(LATE_DRAWS) + 1)
        om = wl.sw_shaped_observation_model()
        idx = list(LATE_DRAWS)
        T_len = FUSED[name][7]
        out = dict(A=b["A"][idx].copy(), B=b["B"][idx].copy(), C=b["C"][idx].copy(), D=b["D"][idx].copy(), sig=b["sigma"][idx].copy(),
                   Z=om["Z"].copy(), y=om["y"][:T_len].copy(), Hdiag=om["Hdiag"].copy())
        refines = None
    elif name == "late_n30":
        sys_ = [wl.sw_shaped_system(LATE30_SEED0 + seed, **LATE30_SHAPE) for seed in LATE30_SEEDS]
        out = dict(A=np.stack([s[0] for s in sys_]), B=np.stack([s[1] for s in sys_]), C=np.stack([s[2] for s in sys_]))
        refines = None
    elif name == "mixed_n30":
        n = 30
        sys_ = [reversal_system(0, n), reversal_system(1, n, scaled=False), reversal_system(2, n, scaled=False),
                reversal_system(3, n, scaled=False), reversal_system(4, n)]
        A, B, C = (np.stack([s[j] for s in sys_]) for j in range(3))
        M = np.eye(n)[::-1] + 0.05 * np.random.default_rng(17199).standard_normal((n, n))
        A[2], B[2], C[2] = M, 0.5 * M, M
        B[3, 3, 4] = np.nan
        out = dict(A=A, B=B, C=C)
        refines = [True, False, False, False, True]
    else:
        n, ns, nl, k, hint, nb, p, T_len = FUSED[name]
        sys_ = [deflatable_system(171000 + 10 * n + i, n, ns, nl, k) for i in range(nb)]
        A, B, C, D = (np.stack([s[j] for s in sys_]) for j in range(4))
        rng = np.random.default_rng(171999 + n)
        Z = np.zeros((p, n))
        Z[np.arange(p), np.arange(p)] = 1.0
        out = dict(A=A, B=B, C=C, D=D, sig=rng.uniform(0.005, 0.02, (nb, k)), Z=Z, y=rng.normal(0, 0.02, (T_len, p)),
                   Hdiag=np.full(p, 1e-4))
        refines = [True] * nb
    for x in out.values():
        x.setflags(write=False)
    out["refines"] = refines
    return out


def input_sha(name):
    a = inputs(name)
    return _sha(*(a[x] for x in ("A", "B", "C", "D", "sig", "Z", "y", "Hdiag") if x in a))


def keys(name):
    if name == "logp_n40":
        return ("logp", "status")
    # (the likelihood call takes the deflated launch only when no iteration counts are asked for)
    return ("T", "R", "status", "logp") if name in FUSED else ("T", "status", "n_iter")


def evaluate(name):
    from geconpy_amd import _frontend as F
    from geconpy_amd import batched

    a = inputs(name)
    if name in FUSED:
        n, ns, nl, k, hint, nb, p, T_len = FUSED[name]
        out = None if name == "logp_n40" else dict(T=np.empty((nb, n, n)), R=np.empty((nb, n, k)))

        def hints(v):
            return dict(n_state_hint=batched.state_hint(v["A"]), z_selector_hint=batched.selector_hint(v["Z"]), n_lead_hint=0)

        r = F.solve_kalman_logp(batched.HOST, a["A"], a["B"], a["C"], a["D"], a["sig"] ** 2, a["Z"], a["y"], d=None, Hdiag=a["Hdiag"],
                                q_mode=1, solver="cycle_reduction", tol=1e-8, max_iter=MAX_ITER, jitter=batched.JITTER_DEFAULT,
                                missing_fill=batched.MISSING_FILL, hints=hints, options={"n_static_hint": hint}, out=out)
        return {key: np.asarray(r[key]) for key in keys(name)}
    if name == "scan_n30":
        T, status, n_iter = batched.scan_cycle_reduction_batched(a["A"], a["B"], a["C"])
    else:
        n = a["A"].shape[1]
        options = {"cr_four_waves": 0} if n > 48 else ({"cr_two_waves": 0} if name == "compact_one_wave" else None)
        T, status, n_iter = batched.cycle_reduction_batched(a["A"], a["B"], a["C"], tol=TOL, max_iter=MAX_ITER, options=options)
    return dict(T=T, status=status, n_iter=n_iter)


def late_candidates(limit=4096):
    """Which bench draws refine late: prints, per draw, the iterations whose pivot ratio is beyond ten times the rule of the
    40-variable tile, for the draws whose first iteration is below the rule itself.  (Host only; slow.)"""
    from geconpy_amd import workloads as wl

    b = wl.sw_shaped_batch(limit)
    for i in range(limit):
        r = host_pivot_ratios(b["A"][i], b["B"][i], b["C"][i], tol=1e-9)
        if r[0] < refine_rule(40) / 10 and (r > 10 * refine_rule(40)).any():
            print(i, np.flatnonzero(r > 10 * refine_rule(40)).tolist(), ["%.1e" % x for x in r], flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "late":
        return late_candidates(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        flat[f"{name}/input_sha256"] = input_sha(name)
        got = evaluate(name)
        for key in keys(name):
            flat[f"{name}/{key}"] = got[key]
        print(name, "status", got["status"].tolist(), "n_iter" if "n_iter" in got else "logp", got.get("n_iter", got.get("logp")).tolist(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
