"""GPU box: record what the tile-layout Kalman filter (kalman_mf_kernel, csrc/dsge_kalman_mf.hpp) returns, bit for bit, at the numbers
of observations tools/make_kalman_mf_bitwise_golden.py does not reach, into tests/golden/kalman_mf_bitwise_p_parent.npz.

    python tools/make_kalman_mf_bitwise_p_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_kalman_mf_bitwise_p.py then compares every array of a later build with np.array_equal.  The F elimination of the
kernel has one code path per number of observations p: pivots 0..6 in one basic block for p >= 7 with pivot 7 behind a branch of
its own (p = 8), a ladder of branches for p < 7.  The other recipe runs p = 3, 4, 5 and 7.  Here, the standalone filter on 4 draws,
T_len = 200, inputs regenerated from seeds and pinned by a SHA-256 of their bytes; every case runs with the steady switch on (logp,
status, first steady step) and with kalman_steady_tol = 0 (logp_full, status_full: 200 full steps), both with dsge_options.mask_d
on: the intercept d is not zero, and with mask_d off every missing entry adds d^2 / jitter ~ 1e8 to the quadratic form -- a
log-likelihood of -6e8, whose last bit is worth 1e-7, hides the roundings this fixture is there to pin:

    kf_p8       p = 8 on 18 state variables (<5,5>): the eighth pivot; whole periods and single entries missing (NaN and the fill marker)
                before the switch and after it, so that the observation mask changes inside the steady loop
    kf_p8_s12   p = 8 on 12 state variables (KT = 3), no observed non-state
    kf_p6       p = 6 on 14 state variables (KT = 4): the last branch of the ladder
    kf_p1       p = 1 on 18 state variables (<5,5>): a single pivot, the observation on a non-state.  (With one observation the gain
                and the downdate are sums of one term, and on 10 or 12 state variables the VALU kernels were seen to return the very
                bits of this kernel -- the fixture could not have said which of them it pins; on 18 they differ)
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kalman_mf_bitwise_p_parent.npz")
T_LEN, NB = 200, 4
# name -> (m, k, p, n_state, seed)
CASES = {"kf_p8": (40, 7, 8, 18, 8308), "kf_p8_s12": (30, 5, 8, 12, 8312), "kf_p6": (36, 6, 6, 14, 8306), "kf_p1": (40, 7, 1, 18, 8401)}


def _base():
    """The recipe this one is modelled on: its checksum and its hook for the first steady step."""
    spec = importlib.util.spec_from_file_location("make_kalman_mf_bitwise_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_bitwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = _base()


def inputs(name):
    from geconpy_amd.batched import MISSING_FILL

    m, k, p, ns, seed = CASES[name]
    rng = np.random.default_rng(seed)
    T = np.zeros((NB, m, m))
    cols = np.sort(rng.choice(m, ns, replace=False))
    for i in range(NB):
        M = rng.standard_normal((m, ns))
        M *= rng.uniform(0.3, 0.95) / np.max(np.abs(np.linalg.eigvals(M[cols])))
        T[i][:, cols] = M
    R = rng.standard_normal((NB, m, k))
    q = rng.uniform(0.5, 1.5, (NB, k))
    Z = np.zeros((p, m))
    others = np.setdiff1d(np.arange(m), cols)
    n_extra = min(1, 4 * ((ns + 3) // 4) - ns)  # one observed non-state where the instance has a spare column for it
    where = np.concatenate([rng.choice(others, n_extra, replace=False), rng.choice(cols, p - n_extra, replace=False)])
    Z[np.arange(p), where] = rng.choice([1.0, 0.25, -2.0], p)
    d = rng.standard_normal(p)
    H = rng.uniform(0.05, 0.5, p)
    y = rng.standard_normal((T_LEN, p))
    last = p - 1
    # before the switch ...
    y[2, 0] = np.nan
    y[5, :] = np.nan
    y[9, last] = MISSING_FILL
    # ... and after it (the steady mode is left, the covariance settles again, the mode is resumed)
    y[120:123, :] = np.nan
    y[150, last] = np.nan
    y[151, 0] = MISSING_FILL
    y[175:178, p // 2] = MISSING_FILL
    y[199, :] = np.nan
    return T, R, q, Z, d, H, y


def run_case(name, extra_options=None):
    """One case on the GPU: dict of arrays.  ``extra_options``: dsge_options fields for both runs (the test uses it to tell the
    kernels apart)."""
    from geconpy_amd import batched

    T, R, q, Z, d, H, y = inputs(name)
    opts = {"mask_d": 1, **(extra_options or {})}
    (lp, st), at = BASE._with_steady_steps(NB, lambda: batched.kalman_logp_batched(T, R, q, Z, y, d=d, Hdiag=H, q_mode="diag_batched",
                                                                                    options=opts))
    lp0, st0 = batched.kalman_logp_batched(T, R, q, Z, y, d=d, Hdiag=H, q_mode="diag_batched",
                                           options={**opts, "kalman_steady_tol": 0.0})
    return dict(input_sha256=BASE._sha(T, R, q, Z, d, H, np.nan_to_num(y, nan=-1.0)), logp=lp, status=st, steady_at=at, logp_full=lp0,
                status_full=st0)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        res = run_case(name)
        print(name, "status", res["status"].tolist(), "steady_at", res["steady_at"].tolist(), "logp", res["logp"].tolist(),
              "logp_full", res["logp_full"].tolist(), flush=True)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
