"""GPU box: record what the FULL step of the tile-layout Kalman filter (kalman_mf_kernel, csrc/dsge_kalman_mf.hpp) returns, bit for
bit, at the smallest shapes that reach every path of it, into tests/golden/kalman_mf_fullstep_parent.npz.

    python tools/make_kalman_mf_fullstep_golden.py [out.npz]
    python tools/make_kalman_mf_fullstep_golden.py --predict      (no GPU: the first steady step a NumPy recursion expects per case)

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_kalman_mf_bitwise_fullstep.py then compares every array of a later build with np.array_equal.  The other three recipes
of this kind run 200 steps of the SW-shaped draws or pin the steady loop; this one pins the full step -- the build of F, the
elimination, the gain and the downdate, the scale of the steady test, the two prediction products -- with short runs (T_LEN steps, NB
draws) of the standalone filter at

    state variables 9, 12, 13, 16, 17, 18, 20       every tile width and both sides of the NS - 2 rule of <5,5> / <5,7>
    observations p = 1, 7, 8                         the per-pivot branches (p < 7), the seven unconditional pivots, the eighth pivot
    retained variables up to 28                      observed NON-states, so that the selected positions lie beyond the state block:
                                                     below lane 16 (9 and 12 state variables) and above it (17, 18, 20)

inputs regenerated from seeds and pinned by a SHA-256 of their bytes.  The data patterns:

    complete   no missing entry: full steps until the covariance has settled, the steady loop to the end
    changing   the missing-data mask CHANGES AT EVERY STEP for the first HOLD_FROM periods (entry t mod p missing; p = 1: every other
               period has no observation at all), then HOLDS (complete data: the full steps run under one mask until the covariance
               has settled, the steady loop starts), changes at LEAVE (one entry missing for three periods: the loop is left), then a
               period with NO observation, a period with ONE observed entry, and complete data again: the loop is entered again

and the special cases:

    tol0            18 state variables, pattern `changing`, kalman_steady_tol = 0: no steady test, no scale, T_LEN full steps
    nonfinite_diag  18 state variables; the measurement variance of entry 0 is +inf in ONE draw (draw 2) and entry 0 is missing for the
                    first NONFINITE_FROM periods (full steps, the mask changing): from then on that draw's F, gain and covariance
                    -- its diagonal included -- are
                    not finite.  Its logp is NaN and its status DSGE_ST_FILTER_NONFINITE; what the steady test makes of such a
                    covariance (`steady_at` of that draw) is pinned as the parent has it.
    rec_grad        the gradient entry on SW-shaped draws 0..3, the first T_LEN periods (forward sweep: the record instance
                    kalman_mf_kernel<5,5,.,REC>, every field of every step's record feeds the cotangents): logp, status, q_bar in
                    full, the other cotangents by their SHA-256; `steady_at` is that of the fused evaluation of the same draws.
    rec_grad_tol0   the same with kalman_steady_tol = 0: T_LEN records of full steps.

Every case must have run at least MIN_FULL full steps, and every case that is about the loop at least MIN_STEADY steady steps in one
stretch: counted from `steady_at` and the masks (the kernel runs full steps up to the period before `steady_at`, then steady steps
while the mask stays what it was), asserted here and again by the test.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kalman_mf_fullstep_parent.npz")
T_LEN, NB, M_FULL, K_SHOCKS = 64, 4, 40, 4  # (40 x 4 doubles of R: what the narrowest instance's W' buffer, 12 x 14, can stage)
STEADY_TOL, MIN_FULL, MIN_STEADY = 1e-8, 8, 8
HOLD_FROM, LEAVE, NONFINITE_FROM = 10, 46, 10
MISSING_FILL = -9999.0  # geconpy_amd.batched.MISSING_FILL (checked in run_case: --predict must not need the library)
STATES, OBS = (9, 12, 13, 16, 17, 18, 20), (1, 7, 8)


def _cases():
    """name -> (state variables, observed non-states, p, data pattern, seed): states x p, the observed non-states as many as the
    instance that holds the state block has room for (4 TM - s, TM = KT + 2 at most) and p allow, the patterns in turn."""
    out = {}
    for i, ns in enumerate(STATES):
        for j, p in enumerate(OBS):
            room = min(4 * ((ns + 3) // 4) + 8, 28) - ns
            n_extra = min(p, room) if (i + j) % 2 == 0 else min(p, room, 1)
            pattern = "complete" if (i + j) % 3 == 0 else "changing"
            out[f"s{ns}_m{ns + n_extra}_p{p}"] = (ns, n_extra, p, pattern, 9100 + 10 * i + j)
    out["tol0"] = (18, 1, 7, "changing", 9180)
    out["nonfinite_diag"] = (18, 1, 7, "complete", 9181)
    return out


CASES = _cases()
NONFINITE_DRAW = 2
EXTRA = ("rec_grad", "rec_grad_tol0")
LOOP_CASES = tuple(n for n, c in CASES.items() if n not in ("tol0", "nonfinite_diag")) + ("rec_grad",)


def _base():
    """The first recipe of this kind: its checksum, its hook for the first steady step, its SW-shaped draws."""
    spec = importlib.util.spec_from_file_location("make_kalman_mf_bitwise_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_bitwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = _base()


def inputs(name):
    ns, n_extra, p, pattern, seed = CASES[name]
    rng = np.random.default_rng(seed)
    T = np.zeros((NB, M_FULL, M_FULL))
    cols = np.sort(rng.choice(M_FULL, ns, replace=False))
    for i in range(NB):
        M = rng.standard_normal((M_FULL, ns))
        # (`changing` mixes fast: the covariance settles between the mask's changes; `complete` slowly: MIN_FULL full steps first)
        M *= rng.uniform(*((0.25, 0.5) if pattern == "changing" else (0.45, 0.65))) / np.max(np.abs(np.linalg.eigvals(M[cols])))
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
    if pattern == "changing":
        for t in range(HOLD_FROM):
            if p > 1 or t % 2 == 1:
                y[t, t % p] = np.nan if t % 3 else MISSING_FILL
        y[LEAVE:LEAVE + 3, p - 1] = np.nan
        y[LEAVE + 3, :] = np.nan           # no observation at all
        y[LEAVE + 4, 1:] = MISSING_FILL    # one observed entry
    if name == "nonfinite_diag":
        H = np.tile(H, (NB, 1))
        H[NONFINITE_DRAW, 0] = np.inf
        y[:NONFINITE_FROM, 0] = np.nan
        y[1:NONFINITE_FROM:2, 1] = np.nan  # (the mask changes at every step until then: no draw turns steady before)
    return T, R, q, Z, d, H, y


def masks(y):
    """Per period: the observed entries as a bit mask."""
    obs = np.isfinite(y) & (y != MISSING_FILL)
    return (obs * (1 << np.arange(y.shape[1]))).sum(axis=1)


def step_counts(mask, steady_at):
    """Per draw: (full steps before the first steady step -- all T_LEN where there is none --, steady steps of the first stretch)."""
    full, stretch = [], []
    for at in np.asarray(steady_at).tolist():
        if at <= 0:
            full.append(len(mask))
            stretch.append(0)
            continue
        n = 0
        while at + n < len(mask) and mask[at + n] == mask[at - 1]:
            n += 1
        full.append(at)
        stretch.append(n)
    return np.array(full), np.array(stretch)


def case_masks(name):
    if name in EXTRA:
        return np.full(T_LEN, 127)  # (complete data, p = 7)
    return masks(inputs(name)[6])


def predict(name, tol=STEADY_TOL, jitter=1e-8):
    """No GPU: the first steady step of every draw by a NumPy covariance recursion with the kernel's rule (the filtered covariance of
    the state block moved by no more than tol x the largest predicted variance).  Roundings differ from the kernel's: this is what the
    cases were CHOSEN with (margins of several steps around MIN_FULL and MIN_STEADY), not what the fixture holds."""
    T, R, q, Z, d, H, y = inputs(name)
    mk = masks(y)
    cols = np.flatnonzero(np.any(T[0] != 0, axis=0))
    out = []
    for i in range(NB):
        Q = (R[i] * q[i]) @ R[i].T
        P, A = Q.copy(), T[i].copy()
        for _ in range(64):
            P, A = P + A @ P @ A.T, A @ A
        Hd = np.broadcast_to(H, (NB, len(d)))[i]
        at, prev = -1, None
        for t in range(T_LEN):
            o = np.flatnonzero((mk[t] >> np.arange(len(d))) & 1)
            Pf = P
            if len(o):
                Zo = Z[o]
                with np.errstate(all="ignore"):
                    F = Zo @ P @ Zo.T + np.diag(Hd[o] + jitter)
                    Pf = P - P @ Zo.T @ np.linalg.solve(F, Zo @ P) if np.isfinite(F).all() else np.full_like(P, np.nan)
            blk = Pf[np.ix_(cols, cols)]
            if t > 0 and tol > 0 and np.max(np.abs(blk - prev)) <= tol * np.max(np.diag(P)):
                at = t + 1
                break
            prev = blk
            P = T[i] @ Pf @ T[i].T + Q
        out.append(at)
    return np.array(out)


def run_case(name, extra_options=None):
    """One case on the GPU: dict of arrays.  ``extra_options``: dsge_options fields on top of the case's own."""
    from geconpy_amd import batched

    assert batched.MISSING_FILL == MISSING_FILL
    tol = 0.0 if name in ("tol0", "rec_grad_tol0") else STEADY_TOL
    opts = {"kalman_steady_tol": tol, **(extra_options or {})}
    if name in EXTRA:
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
    return dict(input_sha256=BASE._sha(T, R, q, Z, d, np.nan_to_num(H, posinf=-2.0), np.nan_to_num(y, nan=-1.0)), logp=lp, status=st,
                steady_at=at)


def check_case(name, res):
    """What a recorded case must show to check anything: see the module's text."""
    full, stretch = step_counts(case_masks(name), res["steady_at"])
    assert (full >= MIN_FULL).all(), (name, "full steps per draw", full.tolist(), res["steady_at"].tolist())
    finite = np.ones(len(res["logp"]), dtype=bool)
    if name == "nonfinite_diag":
        finite[NONFINITE_DRAW] = False
        assert res["status"][NONFINITE_DRAW] == 8 and np.isnan(res["logp"][NONFINITE_DRAW]), (res["status"], res["logp"])
    if name in LOOP_CASES:
        assert (stretch >= MIN_STEADY).all(), (name, "steady steps per draw", stretch.tolist(), res["steady_at"].tolist())
        if name in CASES and CASES[name][3] == "changing":  # the loop starts while the mask holds, and is left at LEAVE
            assert ((res["steady_at"] > HOLD_FROM) & (res["steady_at"] < LEAVE)).all(), (name, res["steady_at"].tolist())
    if name in ("tol0", "rec_grad_tol0"):
        assert (res["steady_at"] == -1).all(), (name, res["steady_at"].tolist())
    assert (res["status"][finite] == 0).all() and np.isfinite(res["logp"][finite]).all(), (name, res["status"], res["logp"])
    assert (np.abs(res["logp"][finite]) < 1e5).all(), (name, res["logp"])  # (of a size at which one rounding shows)


def main():
    if "--predict" in sys.argv:
        for name in CASES:
            at = predict(name, 0.0 if name == "tol0" else STEADY_TOL)
            full, stretch = step_counts(case_masks(name), at)
            print(name, CASES[name], "steady_at", at.tolist(), "full", full.tolist(), "steady", stretch.tolist())
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in tuple(CASES) + EXTRA:
        res = run_case(name)
        full, stretch = step_counts(case_masks(name), res["steady_at"])
        print(name, "status", res["status"].tolist(), "steady_at", res["steady_at"].tolist(), "full steps", full.tolist(),
              "steady steps", stretch.tolist(), "logp", res["logp"].tolist(), flush=True)
        check_case(name, res)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
