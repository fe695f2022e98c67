"""GPU box: record what the steady loop of the tile-layout Kalman filter (kalman_mf_kernel, csrc/dsge_kalman_mf.hpp) returns, bit for
bit, at every width of its mean prediction, into tests/golden/kalman_mf_steady_parent.npz.

    python tools/make_kalman_mf_steady_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_kalman_mf_bitwise_steady.py then compares every array of a later build with np.array_equal.  The steady loop predicts
the mean over NC = NS - 2 or NS columns of the padded state block (NS = 12, 16, 20: one loop body per NC and per instance), on the
lanes of the retained variables m <= 28, and entry kk of the filtered mean sits in 16-lane row kk / 16.  The other two recipes reach
12, 14, 16, 17 and 18 state variables.  Here, short runs (T_LEN steps, NB draws, kalman_steady_tol = 1e-8 and quickly mixing
transitions, so that the loop starts within the first twenty steps) of the standalone filter at

    state variables 9, 10, 11, 12 / 13, 14, 15, 16 / 17, 18, 19, 20     both sides of the NS - 2 rule at every tile width
    retained variables 15, 16, 17 and 28 (and what the state counts force)   below, at and across the row boundary, the maximum
    observations p = 1, 7, 8

inputs regenerated from seeds and pinned by a SHA-256 of their bytes.  The data patterns:

    complete   no missing entry
    no_obs     the first NO_OBS periods have no observation at all: the covariance starts at its stationary value, the loop starts
               at once and runs with NO observation (n_obs = 0), then the mask changes and the full steps take over until the
               covariance has settled again
    reenter    complete until step CHANGE, there one entry missing (NaN) and in the next period another (the fill marker): the loop is
               left, full steps run, the loop is entered again

    rec_grad   the gradient entry on SW-shaped draws 0..3, the first T_LEN periods (forward sweep: the record instance
               kalman_mf_kernel<5,5,.,REC>): logp, status, q_bar in full, the other cotangents by their SHA-256.  The entry does not
               report the first steady step; `steady_at` is that of the fused evaluation of the same draws and data (the same
               covariance recursion).
    nonfinite  s18 with an intercept of +inf in ONE draw (draw 2): its filtered mean is non-finite from the first step on, its
               covariance is not, so it runs the steady loop with the others.  Status bits and logp (NaN there) are recorded.

Every finite case must have run at least MIN_STEADY steady steps in one stretch (from `steady_at` to the first mask change or the
end): asserted here and again by the test.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kalman_mf_steady_parent.npz")
T_LEN, NB, M_FULL, K_SHOCKS = 64, 4, 40, 4  # (40 x 4 doubles of R: what the narrowest instance's W' buffer, 12 x 14, can stage)
STEADY_TOL, MIN_STEADY, NO_OBS, CHANGE = 1e-8, 8, 12, 36
# name -> (state variables, observed non-states, p, data pattern, seed); retained variables m = states + observed non-states
CASES = {
    "s9_m15_p7": (9, 6, 7, "complete", 9001),      # <3,5>, NC = 10
    "s10_m16_p8": (10, 6, 8, "reenter", 9002),     # <3,5>, NC = 10
    "s11_m17_p7": (11, 6, 7, "no_obs", 9003),      # <3,5>, NC = 12
    "s12_m15_p8": (12, 3, 8, "complete", 9004),    # <3,5>, NC = 12
    "s12_m12_p1": (12, 0, 1, "reenter", 9005),     # <3,3>, NC = 12
    "s13_m15_p7": (13, 2, 7, "reenter", 9006),     # <4,4>, NC = 14
    "s14_m16_p8": (14, 2, 8, "no_obs", 9007),      # <4,4>, NC = 14
    "s15_m17_p7": (15, 2, 7, "complete", 9008),    # <4,6>, NC = 16
    "s16_m17_p1": (16, 1, 1, "reenter", 9009),     # <4,6>, NC = 16
    "s16_m16_p8": (16, 0, 8, "complete", 9010),    # <4,4>, NC = 16
    "s17_m17_p1": (17, 0, 1, "no_obs", 9011),      # <5,5>, NC = 18
    "s18_m26_p8": (18, 8, 8, "reenter", 9012),     # <5,7>, NC = 18
    "s19_m20_p7": (19, 1, 7, "complete", 9013),    # <5,5>, NC = 20
    "s20_m28_p8": (20, 8, 8, "reenter", 9014),     # <5,7>, NC = 20
    "s20_m28_p8_no_obs": (20, 8, 8, "no_obs", 9015),
    "nonfinite": (18, 1, 7, "complete", 9016),     # <5,5>, NC = 18
}
NONFINITE_DRAW = 2
EXTRA = ("rec_grad",)


def _base():
    """The first recipe of this kind: its checksum, its hook for the first steady step, its SW-shaped draws."""
    spec = importlib.util.spec_from_file_location("make_kalman_mf_bitwise_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_bitwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = _base()


def first_change(pattern):
    """The first step whose observation mask differs from the one the first steady stretch runs under (T_LEN: none)."""
    return {"complete": T_LEN, "no_obs": NO_OBS, "reenter": CHANGE}[pattern]


def inputs(name):
    from geconpy_amd.batched import MISSING_FILL

    ns, n_extra, p, pattern, seed = CASES[name]
    rng = np.random.default_rng(seed)
    T = np.zeros((NB, M_FULL, M_FULL))
    cols = np.sort(rng.choice(M_FULL, ns, replace=False))
    for i in range(NB):
        M = rng.standard_normal((M_FULL, ns))
        M *= rng.uniform(0.25, 0.5) / np.max(np.abs(np.linalg.eigvals(M[cols])))  # (mixes fast: the covariance settles early)
        T[i][:, cols] = M
    R = rng.standard_normal((NB, M_FULL, K_SHOCKS))
    q = rng.uniform(0.5, 1.5, (NB, K_SHOCKS))
    Z = np.zeros((p, M_FULL))
    others = np.setdiff1d(np.arange(M_FULL), cols)
    where = np.concatenate([rng.choice(others, n_extra, replace=False), rng.choice(cols, p - n_extra, replace=False)])
    Z[np.arange(p), where] = rng.choice([1.0, 0.25, -2.0], p)
    d = rng.standard_normal(p)
    H = rng.uniform(0.05, 0.5, p)
    y = rng.standard_normal((T_LEN, p))
    if pattern == "no_obs":
        y[:NO_OBS, :] = np.nan
    elif pattern == "reenter":
        y[CHANGE, 0] = np.nan
        y[CHANGE + 1, p - 1] = MISSING_FILL
    if name == "nonfinite":
        d = np.tile(d, (NB, 1))
        d[NONFINITE_DRAW, 0] = np.inf
    return T, R, q, Z, d, H, y


def steady_stretch(name, steady_at):
    """Per draw: the steady steps of the first stretch, from the first steady step to the first mask change (or the end)."""
    pattern = "complete" if name in EXTRA else CASES[name][3]
    at = np.asarray(steady_at)
    return np.where(at > 0, first_change(pattern) - at, 0)


def run_case(name, extra_options=None):
    """One case on the GPU: dict of arrays.  ``extra_options``: dsge_options fields on top of the case's own (the test uses it to
    tell the kernels apart)."""
    from geconpy_amd import batched

    opts = {"kalman_steady_tol": STEADY_TOL, **(extra_options or {})}
    if name == "rec_grad":
        from geconpy_amd import workloads as wl

        b = BASE._sw((0, 1, 2, 3))
        om = wl.sw_shaped_observation_model()
        y, q = np.ascontiguousarray(om["y"][:T_LEN]), b["sigma"] ** 2
        sha = BASE._sha(b["A"], b["B"], b["C"], b["D"], b["sigma"], om["Z"], om["Hdiag"], y)
        _, at = BASE._with_steady_steps(4, lambda: batched.solve_kalman_logp_batched(
            b["A"], b["B"], b["C"], b["D"], q, om["Z"], y, Hdiag=om["Hdiag"], q_mode=1, tol=BASE.TOL, max_iter=BASE.MAX_ITER,
            options=opts))
        g = batched.solve_kalman_logp_grad_batched(b["A"], b["B"], b["C"], b["D"], q, om["Z"], y, Hdiag=om["Hdiag"], tol=BASE.TOL,
                                                   max_iter=BASE.MAX_ITER, options=opts)
        return dict(input_sha256=sha, logp=np.asarray(g["logp"]), status=np.asarray(g["status"]), steady_at=at,
                    q_bar=np.asarray(g["q_bar"]), **{f"{k}_sha256": BASE._sha(g[k]) for k in ("A_bar", "B_bar", "C_bar", "D_bar")})
    T, R, q, Z, d, H, y = inputs(name)
    # (mask_d on: the intercept is not zero, and with mask_d off every missing entry adds d^2 / jitter ~ 1e8 to the quadratic form
    #  -- a log-likelihood whose last bit is worth 1e-8 hides the roundings this fixture is there to pin)
    opts = {"mask_d": 1, **opts}
    (lp, st), at = BASE._with_steady_steps(NB, lambda: batched.kalman_logp_batched(T, R, q, Z, y, d=d, Hdiag=H, q_mode="diag_batched",
                                                                                    options=opts))
    return dict(input_sha256=BASE._sha(T, R, q, Z, np.nan_to_num(d, posinf=-2.0), H, np.nan_to_num(y, nan=-1.0)), logp=lp, status=st,
                steady_at=at)


def check_case(name, res):
    """What a recorded case must show to check anything: see the module's text."""
    stretch = steady_stretch(name, res["steady_at"])
    assert (stretch >= MIN_STEADY).all(), (name, "steady steps per draw", stretch.tolist(), res["steady_at"].tolist())
    finite = np.ones(len(res["logp"]), dtype=bool)
    if name == "nonfinite":
        finite[NONFINITE_DRAW] = False
        assert res["status"][NONFINITE_DRAW] != 0 and not np.isfinite(res["logp"][NONFINITE_DRAW]), (res["status"], res["logp"])
    assert (res["status"][finite] == 0).all() and np.isfinite(res["logp"][finite]).all(), (name, res["status"], res["logp"])
    assert (np.abs(res["logp"][finite]) < 1e5).all(), (name, res["logp"])  # (of a size at which one rounding shows)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in tuple(CASES) + EXTRA:
        res = run_case(name)
        print(name, "status", res["status"].tolist(), "steady_at", res["steady_at"].tolist(), "steady steps",
              steady_stretch(name, res["steady_at"]).tolist(), "logp", res["logp"].tolist(), flush=True)
        check_case(name, res)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
