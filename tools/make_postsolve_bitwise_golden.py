"""GPU box: record what the post-solve entries return, bit for bit, into tests/golden/postsolve_bitwise_parent.npz.

    python tools/make_postsolve_bitwise_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_postsolve_bitwise.py then compares every array of a later build bit for bit.  The parity tests of these entries hold
them to numpy references at 1e-9 .. 1e-12; a reordered sum, a moved barrier that happens to be harmless or a different padding passes
there, it cannot pass here.  The entries: impulse responses / FEVD, simulation and forecasts (csrc/dsge_dynamics.hpp), the shock
decomposition (dsge_shock_decomp.hpp), conditional forecasts (dsge_condfc.hpp), the pruned second-order paths (dsge_pruned.hpp),
the smoother (dsge_kalman_smooth.hpp), the simulation smoother (dsge_simsmooth.hpp), the spectral moments (dsge_spectral.hpp) and
the per-step filter outputs (dsge_kalman_out.hpp) -- the kernels that share the pieces of csrc/dsge_postsolve.hpp.

The inputs come from the case tables of the suite (tests/test_gpu_dynamics.py::_case, tests/shock_decomposition_cases.py,
tests/conditional_forecast_cases.py, tests/pruned_dynamics_reference.py, tests/smoother_cases.py, tests/spectral_moments_cases.py)
and from seeded generators here; their bytes are pinned by `<case>/input_sha256`, so that a failing comparison can be told from a
generator that drifted.  Every case has three draws and, where the entry takes a status, DRAW 1 FAILED (ST_NOT_CONVERGED in): the
NaN fill of that draw and what its neighbours get are in the fixture.  An output of at most SMALL bytes is stored in full, a larger
one by the SHA-256 of its bytes (`<key>_sha256`).  Horizons are at most 12 steps unless the case table fixes more.

    sim_<model>_{noshock,full,mid}   simulate: sw17 (m4 != m, k4 != k), sw40 (k = 7, stride 66); 17 paths (a second column group of
                                     one path); n_shock_steps = 0, = n_steps, in between (the K extent switches mid-run); x0 none,
                                     per draw, shared;  sim_sw96: six row tiles, once
    irf_<model>_unit                 unit impulses (S = I) with FEVD, weights per draw; irf_sw96_unit without FEVD
    irf_sw17_c17                     S per draw with c = 17 and weights: the FEVD of more than 16 impulses (dynamics_fevd_kernel)
    fc_<model>_<q layout>            forecast: sw17, sw64; Q diag / diag_batched / full / full_batched; P0 given and null;
                                     covariances off / diag / full; p = 0 and p = 4 with Z, d, Hdiag per draw
    sd_*                             shock decomposition: identity groups (sw17: G = 4; rbc: G = 2) and two groups (sw40: G = 3);
                                     n_paths 1 / 3 / 17; T_len 1 / 2 / 12; remainder on / off; a variable subset; Z shared / per draw
    cf_<name>                        conditional forecast: the named rows of its case table; cf_none: no condition at all
    pr_<model>_{sim,girf,girf_s}     pruned paths: n17, n40; 9 paths (two passes of eight pairs in the GIRF); parts=True;
                                     impulses null and given
    sm_*, ss_*, sp_*, ko_*           smoother, simulation smoother, spectral moments, filter outputs: `_batched` = full Q, Z, d,
                                     Hdiag per draw, `_shared` = one diagonal Q for all draws
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "postsolve_bitwise_parent.npz")
SMALL = 2048  # bytes: an output up to this size is stored in full
NB = 3
FAILED = 1  # the draw that comes in failed


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode() + a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _status():
    from geconpy_amd import _lib

    st = np.zeros(NB, dtype=np.int32)
    st[FAILED] = _lib.ST_NOT_CONVERGED
    return st


def _dyn(name):
    from tests import test_gpu_dynamics as tgd

    return tgd._case(name)


# ---- the cases: name -> function() -> (inputs: list of arrays, outputs: dict of arrays) ------------------------------------------
def _simulate(model, n_paths, n_shock, n_steps, eps_batched, x0_mode, seed):
    def run():
        from geconpy_amd import batched

        T, R, q = _dyn(model)
        m, k = R.shape[1:]
        rng = np.random.default_rng([71, seed])
        eps = rng.standard_normal((NB, n_paths, n_shock, k) if eps_batched else (n_paths, n_shock, k)) * np.sqrt(q[0])
        x0 = None if x0_mode is None else rng.normal(0, 0.01, (n_paths, m) if x0_mode == "shared" else (NB, n_paths, m))
        out = batched.simulate_batched(T, R, eps, n_steps=n_steps, x0=x0, status=_status())
        return [T, R, eps, np.zeros(1) if x0 is None else x0], out
    return run


def _irf(model, c, fevd, n_steps=12):
    def run():
        from geconpy_amd import batched

        T, R, q = _dyn(model)
        k = R.shape[2]
        rng = np.random.default_rng([73, c or 0])
        S = None if c is None else rng.standard_normal((NB, k, c))
        w = None if not fevd else (q if c is None else rng.uniform(0.5, 2.0, c))
        out = batched.impulse_response_batched(T, R, n_steps=n_steps, S=S, weights=w, fevd=fevd, status=_status())
        return [T, R, np.zeros(1) if S is None else S, np.zeros(1) if w is None else w], out
    return run


def _forecast(model, q_mode, with_p0, cov, obs):
    def run():
        from geconpy_amd import batched
        from tests import test_gpu_dynamics as tgd

        T, R, q = _dyn(model)
        f = tgd._forecast_inputs(model)
        k = R.shape[2]
        L = np.random.default_rng([79, k]).normal(0, 0.01, (NB, k, k))
        Qf = L @ L.transpose(0, 2, 1)
        Q = {"diag": q[0], "diag_batched": q, "full": Qf[0], "full_batched": Qf}[q_mode]
        P0 = f["P0"] if with_p0 else None
        Z, d, H = (f["Zdense"], f["d"], f["H"][None] * np.array([1.0, 2.0, 3.0])[:, None]) if obs else (None, None, None)
        out = batched.forecast_batched(T, R, np.ascontiguousarray(Q), f["a0"], P0, n_steps=7, Z=Z, d=d, Hdiag=H, covariances=cov,
                                       q_mode=q_mode, status=_status())
        ins = [T, R, Q, f["a0"]] + [x for x in (P0, Z, d, H) if x is not None]
        return ins, {key: v for key, v in out.items() if v is not None}
    return run


def _decomp(model, n_paths, T_len, groups=None, variables=None, z="shared", remainder=True):
    def run():
        from geconpy_amd import batched
        from tests import shock_decomposition_cases as sc

        T, R = sc.model(model)
        m, k = R.shape[1:]
        e = sc.shocks(NB, n_paths, T_len, k, seed=T_len)
        x = sc.exact_paths(T, R, e, seed=T_len)
        Z = np.eye(2, m) if z == "shared" else np.random.default_rng([83, m]).standard_normal((NB, 2, m))
        out = batched.shock_decomposition_batched(T, R, x, e, groups=groups, variables=variables, Z=Z, remainder=remainder,
                                                  status=_status())
        return [T, R, x, np.nan_to_num(e, nan=-1.0), Z], {key: out[key] for key in ("contributions", "observed")}
    return run


def _condfc(name):
    def run():
        from geconpy_amd import batched
        from tests import conditional_forecast_cases as cc

        if name == "none":  # the inputs of sw17_t0 without its conditions: the baseline paths, no system to solve
            c = cc.case("sw17_t0")
            conditions = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
        else:
            c = cc.case(name)
            conditions = c["conditions"]
        out = batched.conditional_forecast_batched(c["T"], c["R"], c["Q"], c["x0"], conditions, c["n_steps"], status=_status(),
                                                   **cc.kwargs(c))
        ins = [c["T"], c["R"], c["Q"], c["Z"], c["X0"], c["V"]] + [x for x in (c["d"], c["E"]) if x is not None]
        return ins, out
    return run


def _pruned(model, what):
    def run():
        from geconpy_amd import batched
        from tests import pruned_dynamics_reference as pr

        c = pr.case(model)
        sol = pr.solution(c)
        n, k = c["R"].shape[1:]
        rng = np.random.default_rng([89, n])
        eps = rng.standard_normal((NB, 9, 4, k)) * c["sigma"][:, None, None, :]
        x0 = (rng.normal(0, 0.01, (NB, 9, n)), rng.normal(0, 0.001, (NB, 9, n)))
        S = rng.standard_normal((k, 3)) * c["sigma"].mean()
        ins = [c[key] for key in ("T", "R", "g_yy", "g_yu", "g_uu", "g_ss", "S")] + [eps, *x0, S]
        if what == "sim":
            return ins, batched.simulate_pruned_batched(sol, eps, n_steps=12, x0=x0, status=_status(), parts=True)
        if what == "girf":  # unit impulses on 9 baseline paths
            return ins, batched.girf_pruned_batched(sol, n_steps=12, eps=eps, x0=x0, status=_status())
        return ins, batched.girf_pruned_batched(sol, n_steps=12, impulses=S, status=_status())  # given impulses, no baseline shocks
    return run


def _filter_case(form):
    """tests/smoother_cases.py::obs_batched (sw17, three draws; a full Q, Z, d and Hdiag per draw) or, "shared", its model and
    panel with one diagonal Q, Z and Hdiag for all draws."""
    from tests import smoother_cases as smc

    c = smc.case("obs_batched")
    if form == "batched":
        return dict(T=c["T"], R=c["R"], Q=c["q"], q_mode="full_batched", Z=c["Z"], d=c["d"], H=c["H"], y=c["y"])
    return dict(T=c["T"], R=c["R"], Q=np.ascontiguousarray(np.diagonal(c["q"][0])), q_mode="diag", Z=np.ascontiguousarray(c["Z"][0]),
                d=None, H=np.ascontiguousarray(c["H"][0]), y=c["y"])


def _filter_ins(c):
    return [c["T"], c["R"], c["Q"], c["Z"], c["H"], np.nan_to_num(c["y"], nan=-1.0)] + ([] if c["d"] is None else [c["d"]])


def _smoother(form):
    def run():
        from geconpy_amd import batched

        c = _filter_case(form)
        out = batched.kalman_smoother_batched(c["T"], c["R"], c["Q"], c["Z"], c["y"], d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"],
                                              status=_status(), full_covariances=form == "batched")
        return _filter_ins(c), out
    return run


def _filter_outputs(form):
    def run():
        from geconpy_amd import batched

        c = _filter_case(form)
        out = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["Q"], c["Z"], c["y"], d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"],
                                                    status=_status(), full_covariances=form == "batched")
        return _filter_ins(c), out
    return run


def _simsmooth(form):
    def run():
        from geconpy_amd import batched

        c = _filter_case(form)
        n, p = c["y"].shape
        m, k = c["R"].shape[1:]
        rng = np.random.default_rng([97, len(form)])
        x0, eps, eta = rng.normal(0, 0.01, (NB, 3, m)), rng.normal(0, 0.01, (NB, 3, n, k)), rng.normal(0, 0.003, (3, n, p))
        out = batched.simulation_smoother_batched(c["T"], c["R"], c["Q"], c["Z"], c["y"], n_paths=3, d=c["d"], Hdiag=c["H"],
                                                  q_mode=c["q_mode"], x0=x0, eps=eps, eta=eta, status=_status())
        return _filter_ins(c) + [x0, eps, eta], out
    return run


def _spectral(form):
    def run():
        from geconpy_amd import batched
        from tests import spectral_moments_cases as spc

        if form == "batched":  # sw17_band with a full Q and a dense Z per draw (its Hdiag is per draw already)
            kw = dict(spc.case("sw17_band"))
            m, k = kw["R"].shape[1:]
            kw.update(Q=spc._q("sw17_band", k, "full_batched"), q_mode="full_batched", Z=spc._dense_z("sw17_band", 4, m, True))
        else:  # sw40_hp: one diagonal Q, a selector, HP gain
            kw = dict(spc.case("sw40_hp"))
        T, R, Q = kw.pop("T"), kw.pop("R"), kw.pop("Q")
        out = batched.spectral_moments_batched(T, R, Q, status=_status(), **kw)
        ins = [T, R, Q] + [kw[key] for key in ("Z", "Hdiag", "gain") if kw[key] is not None]
        return ins, {key: v for key, v in out.items() if key != "freqs"}
    return run


TWO_GROUPS = [[0, 1, 2], [3, 4, 5, 6]]  # of the 7 shocks of sw40: G = 3 components with the initial condition
_CASES = {}
for _m in ("sw17", "sw40"):
    _CASES[f"sim_{_m}_noshock"] = _simulate(_m, 17, 0, 5, False, "batched", 1)
    _CASES[f"sim_{_m}_full"] = _simulate(_m, 17, 9, 9, True, None, 2)
    _CASES[f"sim_{_m}_mid"] = _simulate(_m, 17, 4, 12, False, "shared", 3)
    _CASES[f"irf_{_m}_unit"] = _irf(_m, None, True)
_CASES["sim_sw96"] = _simulate("sw96", 17, 3, 5, True, "batched", 4)
_CASES["irf_sw96_unit"] = _irf("sw96", None, False, n_steps=5)
_CASES["irf_sw17_c17"] = _irf("sw17", 17, True)
for _m in ("sw17", "sw64"):
    _CASES[f"fc_{_m}_diag"] = _forecast(_m, "diag", False, None, False)
    _CASES[f"fc_{_m}_diag_batched"] = _forecast(_m, "diag_batched", True, "diag", True)
    _CASES[f"fc_{_m}_full"] = _forecast(_m, "full", True, "full", False)
    _CASES[f"fc_{_m}_full_batched"] = _forecast(_m, "full_batched", False, "full", True)
_CASES["sd_sw17_identity"] = _decomp("sw17", 3, 12)
_CASES["sd_sw17_one_period"] = _decomp("sw17", 1, 1, remainder=False)
_CASES["sd_rbc_paths17"] = _decomp("rbc", 17, 2, z="batched")
_CASES["sd_rbc_subset"] = _decomp("rbc", 3, 12, variables=[5, 0, 7], remainder=False)
_CASES["sd_sw40_two_groups"] = _decomp("sw40", 17, 12, groups=TWO_GROUPS, z="batched")
_CASES["sd_sw40_subset"] = _decomp("sw40", 3, 2, groups=TWO_GROUPS, variables=[5, 0, 39], remainder=False)
_CASES["sd_sw40_identity"] = _decomp("sw40", 1, 12)
for _n in ("sw17_gap", "sw17_subset", "sw17_t0", "sw40_last", "sw49_dense", "none"):
    _CASES[f"cf_{_n}"] = _condfc(_n)
for _m in ("n17", "n40"):
    for _w in ("sim", "girf", "girf_s"):
        _CASES[f"pr_{_m}_{_w}"] = _pruned(_m, _w)
for _f in ("batched", "shared"):
    _CASES[f"sm_{_f}"] = _smoother(_f)
    _CASES[f"ss_{_f}"] = _simsmooth(_f)
    _CASES[f"sp_{_f}"] = _spectral(_f)
    _CASES[f"ko_{_f}"] = _filter_outputs(_f)
CASES = tuple(_CASES)


def run_case(name):
    """One case on the GPU: dict(input_sha256, and per output either the array or `<key>_sha256`)."""
    ins, out = _CASES[name]()
    res = dict(input_sha256=_sha(*ins))
    for key, v in out.items():
        if v is None or isinstance(v, list):  # (absent outputs; the component names of the decomposition)
            continue
        v = np.ascontiguousarray(v)
        if v.dtype.kind in "fc" and v.size:  # which draws are NaN throughout: the failed one, and only it
            res[f"{key}_nan_draws"] = np.isnan(v.reshape(NB, -1)).all(axis=1)
        if v.nbytes <= SMALL:
            res[key] = v
        else:
            res[f"{key}_sha256"] = _sha(v)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        res = run_case(name)
        print(name, {k: (v.shape, str(v.dtype)) for k, v in res.items()}, flush=True)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
