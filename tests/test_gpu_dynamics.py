"""GPU: the post-solve dynamics entries (dsge_simulate_batched, dsge_irf_batched, dsge_forecast_batched; csrc/dsge_dynamics.hpp)
against the numpy restatements of tests/dynamics_reference.py and, for the two real models, against what the reference's own
loop gives (tests/golden/dynamics_reference.npz).

Bar: the project's per-step-output bar, 1e-9 x scale, with scale = max|reference| for responses, paths and forecast means,
max|P_h| (max|F_h|) for covariances and 1 for FEVD shares.  The restatement's own deviation from the reference loop is
<= 7e-15 (tests/test_dynamics_reference.py)."""
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import oracle
from geconpy_amd import _lib, batched
from geconpy_amd import workloads as wl

from tests import dynamics_reference as dr

pytestmark = pytest.mark.gpu

BAR = 1e-9
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics_reference.npz"))
SHAPES = {
    "sw17": dict(n=17, n_state=7, n_lead=5, k=3),
    "sw40": {},
    "sw64": dict(n=64, n_state=30, n_lead=20, k=8),
    "sw96": dict(n=96, n_state=40, n_lead=30, k=8),
}
CASES = ["rbc", "full_nk", "sw17", "sw40", "sw64", "sw96"]


def _selection(b, T):
    return np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(T.shape[0])])


@functools.lru_cache(maxsize=None)
def _case(name, nb=3):
    """(T, R, q) of ``nb`` draws (computed once, shared, never modified); draw 0 of the two real models is the golden's."""
    if name in ("rbc", "full_nk"):
        b, _ = (wl.rbc_batch if name == "rbc" else wl.full_nk_batch)(nb)
        T = np.empty_like(b["A"])
        for i in range(nb):
            T[i], ok, _ = oracle.cycle_reduction.cycle_reduction_core(b["A"][i], b["B"][i], b["C"][i], 1000, 1e-12)
            assert ok
        R = _selection(b, T)
        T[0], R[0] = GOLDEN[f"{name}_T"], GOLDEN[f"{name}_R"]
    else:
        b = wl.sw_shaped_batch(nb, **SHAPES[name])
        T = np.ascontiguousarray(b["T_star"])
        R = _selection(b, T)
    q = np.ascontiguousarray(b["sigma"][:nb] ** 2)
    for a in (T, R, q):
        a.setflags(write=False)
    return T, R, q


@functools.lru_cache(maxsize=None)
def _irf_ref(name, n_steps=40):
    T, R, _ = _case(name)
    out = np.stack([dr.impulse_responses(T[i], R[i], n_steps) for i in range(T.shape[0])])
    out.setflags(write=False)
    return out


def _err(got, ref, scale=None):
    scale = np.abs(ref).max() if scale is None else scale
    return np.abs(got - ref).max() / scale


def _report(what, *errs):
    print(what, " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= BAR, (what, errs)


# ---- impulse responses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_irf_unit_impulses(name):
    T, R, _ = _case(name)
    ref = _irf_ref(name)
    errs = []
    for n_steps in (1, 2, 40):
        got = batched.impulse_response_batched(T, R, n_steps=n_steps)["irf"]
        assert got.shape == (3, R.shape[2], n_steps, T.shape[1])
        errs.append(_err(got, ref[:, :, :n_steps], np.abs(ref).max()))
        if n_steps == 40 and name in ("rbc", "full_nk"):
            errs.append(_err(got[0], GOLDEN[f"{name}_irf"]))
    _report(f"irf {name}", *errs)


@pytest.mark.parametrize("name", ["sw17", "sw40", "sw96"])
def test_irf_impulse_matrices(name):
    """S shared and per draw, c = 1, 3 and 17 (the last crosses a column group of 16)."""
    T, R, _ = _case(name)
    k = R.shape[2]
    rng = np.random.default_rng(2)
    errs = []
    for c in (1, 3, 17):
        for S in (rng.standard_normal((k, c)), rng.standard_normal((3, k, c))):
            got = batched.impulse_response_batched(T, R, n_steps=9, S=S)["irf"]
            ref = np.stack([dr.impulse_responses(T[i], R[i], 9, S if S.ndim == 2 else S[i]) for i in range(3)])
            errs.append(_err(got, ref))
    _report(f"irf S {name}", *errs)


# ---- simulate --------------------------------------------------------------------------------------------------------------------
def _sim_ref(T, R, eps, n_steps, x0):
    nb, n_paths = T.shape[0], eps.shape[-3]
    out = np.empty((nb, n_paths, n_steps, T.shape[1]))
    for i in range(nb):
        for s in range(n_paths):
            e = eps[s] if eps.ndim == 3 else eps[i, s]
            x = None if x0 is None else (x0[s] if x0.ndim == 2 else x0[i, s])
            out[i, s] = dr.propagate(T[i], R[i], e, n_steps, x)
    return out


@pytest.mark.parametrize("name", ["sw17", "sw40", "sw96"])
def test_simulate_parity(name):
    T, R, q = _case(name)
    m, k = R.shape[1:]
    rng = np.random.default_rng(7)
    errs = []
    for n_paths, n_shock, n_steps, eps_b, x0_mode in ((1, 1, 6, False, None), (16, 4, 9, True, "shared"), (17, 9, 9, False, "batched"),
                                                      (17, 3, 5, True, None), (16, 5, 5, False, None)):
        eps = rng.standard_normal((3, n_paths, n_shock, k) if eps_b else (n_paths, n_shock, k)) * np.sqrt(q[0])
        x0 = None if x0_mode is None else rng.normal(0, 0.01, (n_paths, m) if x0_mode == "shared" else (3, n_paths, m))
        got = batched.simulate_batched(T, R, eps, n_steps=n_steps, x0=x0)["paths"]
        errs.append(_err(got, _sim_ref(T, R, eps, n_steps, x0)))
    _report(f"simulate {name}", *errs)


@pytest.mark.parametrize("name", ["rbc", "full_nk"])
def test_simulate_golden_trajectory(name):
    T, R, _ = _case(name)
    got = batched.simulate_batched(T, R, GOLDEN[f"{name}_shocks"][None])["paths"]
    _report(f"trajectory {name}", _err(got[0, 0], GOLDEN[f"{name}_path"]))


def test_irf_entry_equals_simulate_with_the_same_shocks():
    T, R, _ = _case("sw40")
    k = R.shape[2]
    S = np.random.default_rng(4).standard_normal((k, 5))
    irf = batched.impulse_response_batched(T, R, n_steps=12, S=S)["irf"]
    sim = batched.simulate_batched(T, R, np.ascontiguousarray(S.T)[:, None, :], n_steps=12)["paths"]
    _report("irf vs simulate", _err(irf, sim))


# ---- FEVD ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full_nk", "sw40", "sw96"])
def test_fevd_parity(name):
    T, R, q = _case(name)
    k = R.shape[2]
    ref_irf = _irf_ref(name)
    errs = []
    for w in (None, q[0], q):
        out = batched.impulse_response_batched(T, R, n_steps=40, weights=w, fevd=True)
        ref = np.stack([dr.fevd(ref_irf[i], None if w is None else (w if w.ndim == 1 else w[i])) for i in range(3)])
        assert out["fevd"].shape == (3, 40, T.shape[1], k)
        assert np.abs(out["fevd"].sum(axis=3) - 1.0).max() <= BAR
        errs += [_err(out["fevd"], ref, 1.0), _err(out["irf"], ref_irf)]
        alone = batched.impulse_response_batched(T, R, n_steps=40, weights=w, fevd=True, irf=False)
        assert alone["irf"] is None
        assert_array_equal(alone["fevd"], out["fevd"])
    _report(f"fevd {name}", *errs)


def test_fevd_of_more_than_sixteen_impulses():
    """c = 17: the second pass over the stored responses -- with the responses requested and, alone, through library scratch."""
    T, R, _ = _case("sw17")
    rng = np.random.default_rng(8)
    S, w = rng.standard_normal((3, 3, 17)), rng.uniform(0.5, 2.0, 17)
    out = batched.impulse_response_batched(T, R, n_steps=10, S=S, weights=w, fevd=True)
    ref_irf = np.stack([dr.impulse_responses(T[i], R[i], 10, S[i]) for i in range(3)])
    ref = np.stack([dr.fevd(ref_irf[i], w) for i in range(3)])
    alone = batched.impulse_response_batched(T, R, n_steps=10, S=S, weights=w, fevd=True, irf=False)
    assert_array_equal(alone["fevd"], out["fevd"])
    assert np.abs(out["fevd"].sum(axis=3) - 1.0).max() <= BAR
    _report("fevd c=17", _err(out["fevd"], ref, 1.0), _err(out["irf"], ref_irf))


def test_fevd_of_a_variable_nothing_moves_is_nan_in_its_rows_only():
    T, R, _ = _case("sw17")
    T, R = T.copy(), R.copy()
    T[1, 4], R[1, 4] = 0.0, 0.0  # draw 1: variable 4 has a zero row in both
    out = batched.impulse_response_batched(T, R, n_steps=8, fevd=True)
    ref = np.stack([dr.fevd(dr.impulse_responses(T[i], R[i], 8)) for i in range(3)])
    nan = np.zeros(ref.shape, dtype=bool)
    nan[1, :, 4, :] = True
    assert_array_equal(np.isnan(out["fevd"]), nan)
    assert_array_equal(np.isnan(ref), nan)
    _report("fevd zero row", _err(out["fevd"][~nan], ref[~nan], 1.0))


# ---- forecast --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forecast_inputs(name):
    T, R, q = _case(name)
    m = T.shape[1]
    rng = np.random.default_rng(9)
    a0 = rng.normal(0, 0.01, (3, m))
    M = rng.normal(0, 0.01, (3, m, m))
    P0 = M @ np.transpose(M, (0, 2, 1))
    Zd = rng.standard_normal((3, 4, m)) * (rng.random((3, 4, m)) < 0.3)
    return dict(a0=a0, P0=P0, Zsel=np.eye(4, m, 2), Zdense=Zd, d=rng.normal(0, 0.01, (3, 4)), H=rng.uniform(1e-5, 1e-4, 4))


def _forecast_errs(got, ref_list, full):
    errs = []
    for key in ("states", "covs", "observed", "observed_covs"):
        if got[key] is None:
            continue
        ref = np.stack([r[key] for r in ref_list])
        if key == "covs" and not full:
            ref = np.diagonal(ref, axis1=2, axis2=3)
            scale = np.abs(np.stack([r["covs"] for r in ref_list])).max()
        else:
            scale = np.abs(ref).max()
        errs.append(_err(got[key], ref, scale))
    return errs


@pytest.mark.parametrize("name", ["sw17", "sw40", "sw64"])
def test_forecast_parity(name):
    T, R, q = _case(name)
    f = _forecast_inputs(name)
    errs = []
    for obs, cov, with_p0 in (("none", "full", True), ("none", None, True), ("sel", "diag", True), ("dense", "full", True),
                              ("dense", "diag", False), ("sel", None, False)):
        Z = {"none": None, "sel": f["Zsel"], "dense": f["Zdense"]}[obs]
        d, H = (f["d"], f["H"]) if obs == "dense" else (None, None)
        P0 = f["P0"] if with_p0 else None
        got = batched.forecast_batched(T, R, q, f["a0"], P0, n_steps=7, Z=Z, d=d, Hdiag=H, covariances=cov, q_mode="diag_batched")
        ref = [dr.forecast(T[i], R[i], q[i], f["a0"][i], None if P0 is None else P0[i], 7, None if Z is None else (Z if Z.ndim == 2 else Z[i]),
                           None if d is None else d[i], H) for i in range(3)]
        assert (got["covs"] is None) == (cov is None) and (got["observed"] is None) == (Z is None)
        assert (got["observed_covs"] is None) == (Z is None or cov is None)
        errs += _forecast_errs(got, ref, cov == "full")
    # a full shock covariance, shared
    L = np.random.default_rng(1).normal(0, 0.01, (R.shape[2], R.shape[2]))
    Q = L @ L.T
    got = batched.forecast_batched(T, R, Q, f["a0"], f["P0"], n_steps=3, covariances="full", q_mode="full")
    errs += _forecast_errs(got, [dr.forecast(T[i], R[i], Q, f["a0"][i], f["P0"][i], 3) for i in range(3)], True)
    _report(f"forecast {name}", *errs)


def test_one_step_forecast_from_the_device_filter_is_its_next_prediction():
    T, R, q = _case("sw40")
    om = wl.sw_shaped_observation_model()
    filt = batched.kalman_filter_outputs_batched(T, R, q, om["Z"], om["y"][:8], Hdiag=om["Hdiag"], full_covariances=True)
    assert (filt["status"] == 0).all()
    errs = []
    for t in (0, 3, 6):
        got = batched.forecast_batched(T, R, q, filt["filtered_states"][:, t], filt["filtered_covs"][:, t], n_steps=1,
                                       covariances="full", q_mode="diag_batched")
        errs += [_err(got["states"][:, 0], filt["predicted_states"][:, t + 1], np.abs(filt["predicted_states"]).max()),
                 _err(got["covs"][:, 0], filt["predicted_covs"][:, t + 1], np.abs(filt["predicted_covs"]).max())]
    _report("forecast from filter", *errs)


def test_forecast_beyond_64_variables_is_refused_with_the_outputs_untouched():
    lib = _lib.load()
    p = lambda x: x.ctypes.data  # noqa: E731
    T, R, q, a0 = np.zeros((1, 65, 65)), np.zeros((1, 65, 2)), np.ones(2), np.zeros((1, 65))
    a, P = np.full((1, 3, 65), 7.0), np.full((1, 3, 65), 7.0)
    rc = lib.dsge_forecast_batched_host(p(T), p(R), p(q), 0, None, 0, None, 0, None, 0, p(a0), None, None, 1, 65, 2, 0, 3, p(a), p(P), 0,
                                        None, None)
    assert rc == _lib.ERR_TOO_LARGE
    assert (a == 7.0).all() and (P == 7.0).all()
    with pytest.raises(_lib.DsgeTooLargeError):
        batched.forecast_batched(T, R, q, a0, n_steps=3)


# ---- failed draw, edges, engine --------------------------------------------------------------------------------------------------
def test_failed_draw_is_nan_and_leaves_its_neighbours_alone():
    T, R, q = _case("sw40")
    f = _forecast_inputs("sw40")
    st = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32)
    eps = np.random.default_rng(3).standard_normal((17, 5, R.shape[2]))
    calls = {
        "simulate": lambda s: batched.simulate_batched(T, R, eps, n_steps=8, status=s),
        "irf": lambda s: batched.impulse_response_batched(T, R, n_steps=8, fevd=True, status=s),
        "forecast": lambda s: batched.forecast_batched(T, R, q, f["a0"], f["P0"], n_steps=5, Z=f["Zdense"], d=f["d"], Hdiag=f["H"],
                                                       covariances="full", q_mode="diag_batched", status=s),
    }
    for name, call in calls.items():
        good, mixed = call(None), call(st)
        for key, g in good.items():
            assert np.isfinite(g).all(), (name, key)
            assert np.isnan(mixed[key][1]).all(), (name, key)
            assert_array_equal(mixed[key][[0, 2]], g[[0, 2]], err_msg=f"{name} {key}")
    assert_array_equal(st, [0, _lib.ST_NOT_CONVERGED, 0])  # (input only)


def test_edges():
    T, R, q = _case("sw17")
    lib = _lib.load()
    p = lambda x: x.ctypes.data  # noqa: E731
    eps = np.zeros((2, 4, 3))
    a0 = np.zeros((3, 17))
    guard = np.full(8, 7.0)
    # zero batch, zero steps, zero paths: success, nothing touched
    for nb, n_paths, n_steps, n_shock in ((0, 2, 4, 4), (3, 2, 0, 0), (3, 0, 4, 4)):
        assert lib.dsge_simulate_batched_host(p(T), p(R), p(eps), 0, None, 0, None, nb, 17, 3, n_paths, n_steps, n_shock, p(guard)) == 0
    for nb, n_steps in ((0, 4), (3, 0)):
        assert lib.dsge_irf_batched_host(p(T), p(R), None, 0, None, 0, None, nb, 17, 3, 3, n_steps, p(guard), p(guard)) == 0
        assert lib.dsge_forecast_batched_host(p(T), p(R), p(q), 1, None, 0, None, 0, None, 0, p(a0), None, None, nb, 17, 3, 0, n_steps,
                                              p(guard), p(guard), 0, None, None) == 0
    assert (guard == 7.0).all()
    assert batched.simulate_batched(T, R, np.zeros((0, 4, 3)))["paths"].shape == (3, 0, 4, 17)
    assert batched.impulse_response_batched(T, R, n_steps=0, fevd=True)["fevd"].shape == (3, 0, 17, 3)
    assert batched.forecast_batched(T[:0], R[:0], q[:0], a0[:0], n_steps=2, q_mode="diag_batched")["states"].shape == (0, 2, 17)
    # malformed calls
    bad = _lib.ERR_INVALID
    out = np.empty((3, 2, 4, 17))
    assert lib.dsge_simulate_batched_host(None, p(R), p(eps), 0, None, 0, None, 3, 17, 3, 2, 4, 4, p(out)) == bad
    assert lib.dsge_simulate_batched_host(p(T), p(R), None, 0, None, 0, None, 3, 17, 3, 2, 4, 4, p(out)) == bad
    assert lib.dsge_simulate_batched_host(p(T), p(R), p(eps), 0, None, 0, None, 3, 17, 3, 2, 4, 4, None) == bad
    assert lib.dsge_simulate_batched_host(p(T), p(R), p(eps), 0, None, 0, None, 3, 17, 3, 2, 3, 4, p(out)) == bad  # n_shock_steps > n_steps
    assert lib.dsge_irf_batched_host(p(T), None, None, 0, None, 0, None, 3, 17, 3, 3, 4, p(out), None) == bad
    assert lib.dsge_irf_batched_host(p(T), p(R), None, 0, None, 0, None, 3, 17, 3, 3, 4, None, None) == bad   # no output
    assert lib.dsge_irf_batched_host(p(T), p(R), None, 0, None, 0, None, 3, 17, 3, 2, 4, p(out), None) == bad  # S = I needs c = k
    assert lib.dsge_forecast_batched_host(p(T), p(R), p(q), 1, None, 0, None, 0, None, 0, None, None, None, 3, 17, 3, 0, 4, p(out), None, 0,
                                          None, None) == bad  # a0
    assert lib.dsge_forecast_batched_host(p(T), p(R), None, 1, None, 0, None, 0, None, 0, p(a0), None, None, 3, 17, 3, 0, 4, p(out), p(out),
                                          0, None, None) == bad  # covariances without Q
    assert lib.dsge_forecast_batched_host(p(T), p(R), p(q), 1, None, 0, None, 0, None, 0, p(a0), None, None, 3, 17, 3, 0, 4, None, None, 0,
                                          None, None) == bad  # no output
    assert lib.dsge_simulate_batched_host(p(T), p(R), p(eps), 0, None, 0, None, 1, 97, 3, 2, 4, 4, p(out)) == _lib.ERR_TOO_LARGE


def test_engine_equals_host_twin_on_a_side_stream():
    import torch
    from geconpy_amd.engine import LogpEngine

    T, R, q = _case("sw40")
    f = _forecast_inputs("sw40")
    k = R.shape[2]
    rng = np.random.default_rng(6)
    eps, x0, S = rng.standard_normal((3, 17, 5, k)), rng.normal(0, 0.01, (17, 40)), rng.standard_normal((k, 5))
    ref_sim = batched.simulate_batched(T, R, eps, n_steps=9, x0=x0)["paths"]
    ref_irf = batched.impulse_response_batched(T, R, n_steps=12, S=S, weights=q[:, :5], fevd=True)
    ref_fc = batched.forecast_batched(T, R, q, f["a0"], f["P0"], n_steps=6, Z=f["Zdense"], d=f["d"], Hdiag=f["H"], covariances="full",
                                      q_mode="diag_batched")
    eng = LogpEngine(0)
    dev = lambda x: eng.to_device(np.array(x))  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Td, Rd = dev(T), dev(R)
        sim = eng.simulate(Td, Rd, dev(eps), n_steps=9, x0=dev(x0))
        irf = eng.impulse_response(Td, Rd, n_steps=12, S=dev(S), weights=dev(q[:, :5]), fevd=True)
        fc = eng.forecast(Td, Rd, dev(q), dev(f["a0"]), dev(f["P0"]), n_steps=6, Z=dev(f["Zdense"]), d=dev(f["d"]), Hdiag=dev(f["H"]),
                          covariances="full", q_mode=1)
        pre = torch.empty((3, k, 4, 40), dtype=torch.float64, device=eng.device)
        assert eng.impulse_response(Td, Rd, n_steps=4, out=dict(irf=pre))["irf"] is pre
    side.synchronize()
    assert_array_equal(sim.cpu().numpy(), ref_sim)
    for key in ("irf", "fevd"):
        assert_array_equal(irf[key].cpu().numpy(), ref_irf[key], err_msg=key)
    for key in ("states", "covs", "observed", "observed_covs"):
        assert_array_equal(fc[key].cpu().numpy(), ref_fc[key], err_msg=key)
    assert_array_equal(pre.cpu().numpy(), batched.impulse_response_batched(T, R, n_steps=4)["irf"])


def test_unit_impulses_of_2048_draws():
    """Grid and indexing at a batch far beyond the device's resident workgroups: 2 048 default SW draws, 40 steps, checked on 16
    sampled draws (first, last and 14 in between)."""
    b = wl.sw_shaped_batch(2048)
    T = np.ascontiguousarray(b["T_star"])
    R = _selection(b, T)
    got = batched.impulse_response_batched(T, R, n_steps=40)["irf"]
    assert np.isfinite(got).all()
    pick = np.unique(np.concatenate([[0, 2047], np.random.default_rng(0).integers(1, 2047, 14)]))
    errs = [_err(got[i], dr.impulse_responses(T[i], R[i], 40)) for i in pick]
    _report("irf 2048", max(errs))
