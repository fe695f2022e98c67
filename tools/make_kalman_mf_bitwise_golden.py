"""GPU box: record what the tile-layout Kalman filter (kalman_mf_kernel, csrc/dsge_kalman_mf.hpp) returns, bit for bit, into
tests/golden/kalman_mf_bitwise_parent.npz.

    python tools/make_kalman_mf_bitwise_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_kalman_mf_bitwise.py then compares every array of a later build with np.array_equal.  The parity tests of the suite
compare this kernel with the VALU kernels to 1e-11; a change of the order of two floating-point operations passes there, it cannot
pass here.

The inputs are regenerated from seeds and pinned by a SHA-256 of their bytes (`<case>/input_sha256`), so that a failing comparison can
be told from a generator that drifted.  Every case runs T_len = 200 steps, so that the steady loop runs where it may.  Cases:

    sw_fused            SW-shaped draws 0..3, fused evaluation, kalman_mf_kernel<5,5>: logp, status, first steady step
    sw_never_steady     draw 3437 (never steady: 200 full steps) and draw 752 (the refining draw)
    sw_jumps            draws 0..3, 3437, 752 with observed jump variables (SW_OBSERVED_JUMPS): the <5,7> second pass
    sw_full_recursion   draws 0..3 with kalman_steady_tol = 0: no steady loop, every step full
    sw_nan10            10 % of y missing, scattered: the mask changes nearly every step
    sw_missing_block    whole periods and single entries missing after the switch: the steady mode is left and resumed
    sw_d_mask_on/_off   d != 0 on the data of sw_missing_block, dsge_options.mask_d on and off
    sw_conventions      jitter_F on, jitter_P off, joseph off, ll_constant "observed", on the data of sw_missing_block
    kf_s12, kf_s16      the standalone filter on 12 state variables (KT = 3) and 16 (KT = 4), observed non-states, NaN and fill markers
    kf_p3               the standalone filter with p = 3 (the elimination that keeps its per-pivot branches)
    rec_outputs         kalman_filter_outputs_batched on draws 0, 1: ll_t and the filtered moments in full, the predicted moments by
                        their SHA-256
    rec_grad            the gradient entry on draws 0..3 (forward sweep: the record instance kalman_mf_kernel<5,5,.,REC>): logp, status,
                        q_bar in full and the other cotangents -- every record field feeds them -- by their SHA-256
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kalman_mf_bitwise_parent.npz")
TOL, MAX_ITER, T_LEN = 1e-8, 1000, 200
# name -> (m, k, p, n_state, seed): shapes of tests/test_gpu_parity.py::test_kalman_mf_kernel_matches_valu_kernels
STANDALONE = {"kf_s12": (30, 5, 4, 12, 8112), "kf_s16": (36, 6, 5, 16, 8116), "kf_p3": (40, 7, 3, 17, 8103)}
CASES = ("sw_fused", "sw_never_steady", "sw_jumps", "sw_full_recursion", "sw_nan10", "sw_missing_block", "sw_d_mask_on",
         "sw_d_mask_off", "sw_conventions") + tuple(STANDALONE) + ("rec_outputs", "rec_grad")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _sw(draws):
    """SW-shaped systems of the listed draws, stacked."""
    from geconpy_amd import workloads as wl

    parts = [wl.sw_shaped_batch(1, first_draw=i) for i in draws]
    return {k: np.concatenate([q[k] for q in parts]) for k in ("A", "B", "C", "D", "sigma")}


def _y_nan10(y):
    y = y.copy()
    y[np.random.default_rng(8201).random(y.shape) < 0.10] = np.nan
    return y


def _y_block(y):
    """Missing data after the steady switch (step 30 .. 40 on these draws): ten whole periods, then single entries, then a fill marker."""
    from geconpy_amd.batched import MISSING_FILL

    y = y.copy()
    y[90:100, :] = np.nan
    y[120:125, 2] = np.nan
    y[150, 0] = MISSING_FILL
    y[151, :] = MISSING_FILL
    return y


def _standalone_inputs(name):
    from geconpy_amd.batched import MISSING_FILL

    m, k, p, ns, seed = STANDALONE[name]
    nb = 4
    rng = np.random.default_rng(seed)
    T = np.zeros((nb, m, m))
    cols = np.sort(rng.choice(m, ns, replace=False))
    for i in range(nb):
        M = rng.standard_normal((m, ns))
        M *= rng.uniform(0.3, 0.95) / np.max(np.abs(np.linalg.eigvals(M[cols])))
        T[i][:, cols] = M
    R = rng.standard_normal((nb, m, k))
    q = rng.uniform(0.5, 1.5, (nb, k))
    Z = np.zeros((p, m))
    # one observed non-state where the instance has room for it (4 KT - ns spare columns), the rest on states
    others = np.setdiff1d(np.arange(m), cols)
    n_extra = min(1, 4 * ((ns + 3) // 4) - ns)
    where = np.concatenate([rng.choice(others, n_extra, replace=False), rng.choice(cols, p - n_extra, replace=False)])
    Z[np.arange(p), where] = rng.choice([1.0, 0.25, -2.0], p)
    d = rng.standard_normal(p)
    H = rng.uniform(0.05, 0.5, p)
    y = rng.standard_normal((T_LEN, p))
    y[2, 0] = np.nan
    y[5, :] = np.nan
    y[9, 1:3] = MISSING_FILL
    y[130:134, :] = np.nan
    y[160, 1] = np.nan
    return T, R, q, Z, d, H, y


def _with_steady_steps(nb, fn):
    """fn() with the first steady step of every draw recorded (int32, -1 = never)."""
    import torch

    from geconpy_amd import _lib

    lib = _lib.load()
    at = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    _lib.check(lib.dsge_debug_kalman_steady_steps(at.data_ptr()))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.dsge_debug_kalman_steady_steps(None))
    return out, at.cpu().numpy()


def run_case(name, extra_options=None):
    """One case on the GPU: dict of arrays (inputs' checksum + everything the entry point returned).  ``extra_options``: dsge_options
    fields on top of the case's own (the fused SW-shaped cases only; the test uses it to tell the kernels apart)."""
    from geconpy_amd import batched
    from geconpy_amd import workloads as wl

    if name in STANDALONE:
        T, R, q, Z, d, H, y = _standalone_inputs(name)
        (lp, st), at = _with_steady_steps(len(T), lambda: batched.kalman_logp_batched(T, R, q, Z, y, d=d, Hdiag=H,
                                                                                      q_mode="diag_batched"))
        (lp0, st0) = batched.kalman_logp_batched(T, R, q, Z, y, d=d, Hdiag=H, q_mode="diag_batched", options={"kalman_steady_tol": 0.0})
        return dict(input_sha256=_sha(T, R, q, Z, d, H, np.nan_to_num(y, nan=-1.0)), logp=lp, status=st, steady_at=at,
                    logp_full=lp0, status_full=st0)

    draws = {"sw_never_steady": (3437, 752), "sw_jumps": (0, 1, 2, 3, 3437, 752), "rec_outputs": (0, 1)}.get(name, (0, 1, 2, 3))
    b = _sw(draws)
    om = wl.sw_shaped_observation_model(observed=wl.SW_OBSERVED_JUMPS) if name == "sw_jumps" else wl.sw_shaped_observation_model()
    y, d, options = om["y"], None, None
    if name == "sw_nan10":
        y = _y_nan10(y)
    elif name in ("sw_missing_block", "sw_d_mask_on", "sw_d_mask_off", "sw_conventions"):
        y = _y_block(y)
    if name.startswith("sw_d_mask"):
        d = 0.01 * np.random.default_rng(8202).standard_normal(y.shape[1])
        options = {"mask_d": int(name.endswith("_on"))}
    elif name == "sw_conventions":
        from geconpy_amd import _lib

        options = _lib.filter_conventions(ll_constant="observed", jitter_on_F=True, jitter_on_P=False, mask_d=False, joseph=False)
    elif name == "sw_full_recursion":
        options = {"kalman_steady_tol": 0.0}
    if extra_options:
        options = {**(options or {}), **extra_options}
    q = b["sigma"] ** 2
    sha = _sha(b["A"], b["B"], b["C"], b["D"], b["sigma"], om["Z"], om["Hdiag"], np.nan_to_num(y, nan=-1.0),
               np.zeros(1) if d is None else d)
    if name == "rec_grad":
        g = batched.solve_kalman_logp_grad_batched(b["A"], b["B"], b["C"], b["D"], q, om["Z"], y, Hdiag=om["Hdiag"], tol=TOL,
                                                   max_iter=MAX_ITER)
        return dict(input_sha256=sha, logp=np.asarray(g["logp"]), status=np.asarray(g["status"]), q_bar=np.asarray(g["q_bar"]),
                    **{f"{k}_sha256": _sha(g[k]) for k in ("A_bar", "B_bar", "C_bar", "D_bar")})
    if name == "rec_outputs":
        r = batched.solve_kalman_logp_batched(b["A"], b["B"], b["C"], b["D"], q, om["Z"], y, Hdiag=om["Hdiag"], q_mode=1, tol=TOL,
                                              max_iter=MAX_ITER, return_policy=True)
        assert (r["status"] == 0).all(), r["status"]
        o = batched.kalman_filter_outputs_batched(r["T"], r["R"], q, om["Z"], y, Hdiag=om["Hdiag"], q_mode="diag_batched")
        return dict(input_sha256=sha, status=o["status"], ll=o["ll"], filtered_states=o["filtered_states"],
                    filtered_covs=o["filtered_covs"], predicted_states_sha256=_sha(o["predicted_states"]),
                    predicted_covs_sha256=_sha(o["predicted_covs"]))
    r, at = _with_steady_steps(len(draws), lambda: batched.solve_kalman_logp_batched(
        b["A"], b["B"], b["C"], b["D"], q, om["Z"], y, d=d, Hdiag=om["Hdiag"], q_mode=1, tol=TOL, max_iter=MAX_ITER, options=options))
    return dict(input_sha256=sha, logp=r["logp"], status=r["status"], steady_at=at)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        res = run_case(name)
        print(name, {k: (v.shape, str(v.dtype)) for k, v in res.items()}, "status", res["status"].tolist(),
              "steady_at", res["steady_at"].tolist() if "steady_at" in res else None, "logp",
              res["logp"].tolist() if "logp" in res else None, flush=True)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
