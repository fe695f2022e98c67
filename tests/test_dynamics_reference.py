"""CPU: the numpy restatements of the post-solve dynamics (tests/dynamics_reference.py) against what the reference's own loop
gives (tests/golden/dynamics_reference.npz), against the oracle's stationary covariance and against the oracle filter's own
prediction step; and the shape checks of the three numpy wrappers (no GPU needed: they run before anything is staged)."""
import os

import numpy as np
import pytest

import oracle
from geconpy_amd import batched

from tests import dynamics_reference as dr

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics_reference.npz"))


def _model(name):
    return GOLDEN[f"{name}_T"], GOLDEN[f"{name}_R"]


@pytest.mark.parametrize("model", ["rbc", "full_nk"])
def test_restatement_equals_the_reference_loop(model):
    """Unit impulses over 40 periods and one trajectory-mode run: 1e-13 x max|irf| (measured: <= 7e-15)."""
    T, R = _model(model)
    irf = dr.impulse_responses(T, R, 40)
    path = dr.propagate(T, R, GOLDEN[f"{model}_shocks"])
    scale = np.abs(GOLDEN[f"{model}_irf"]).max()
    errs = (np.abs(irf - GOLDEN[f"{model}_irf"]).max() / scale,
            np.abs(path - GOLDEN[f"{model}_path"]).max() / np.abs(GOLDEN[f"{model}_path"]).max())
    print(model, errs)
    assert max(errs) <= 1e-13, errs


@pytest.mark.parametrize("model", ["rbc", "full_nk"])
def test_fevd_rows_sum_to_one(model):
    T, R = _model(model)
    k = R.shape[1]
    w = np.linspace(0.5, 2.0, k)
    for weights in (None, w):
        f = dr.fevd(dr.impulse_responses(T, R, 40), weights)
        assert f.shape == (40, T.shape[0], k)
        assert np.isfinite(f).all() and (f >= 0).all()  # (no row of R is identically zero)
        assert np.abs(f.sum(axis=2) - 1.0).max() <= 1e-14
    # a variable nothing moves: NaN in exactly its rows
    T2, R2 = T.copy(), R.copy()
    T2[2], R2[2] = 0.0, 0.0
    f = dr.fevd(dr.impulse_responses(T2, R2, 5))
    assert np.isnan(f[:, 2]).all() and np.isfinite(np.delete(f, 2, axis=1)).all()


def test_both_recursions_reach_the_stationary_covariance():
    """RBC (draw 0: rho(T) = 0.951, so the tail beyond 400 steps is rho^800 = 4e-18 of the sum): the unnormalised FEVD total sum_j q_j sum_s irf_j[s]^2 and the forecast's diag(P_h)
    from P0 = 0 are both partial sums of sum_s T^s R Q R' T'^s, whose limit the oracle's Lyapunov solve gives: 1e-8 relative,
    entry by entry."""
    T, R = _model("rbc")
    assert np.abs(np.linalg.eigvals(T)).max() ** 800 < 1e-12  # (the truncation is far below the bar)
    q = np.array([0.01 ** 2])
    Sigma = oracle.solve_discrete_lyapunov(T, R @ np.diag(q) @ R.T)
    total = dr.fevd_totals(dr.impulse_responses(T, R, 400), q)[-1].sum(axis=1)
    fc = dr.forecast(T, R, q, np.zeros(T.shape[0]), None, 400)
    e1 = np.abs(total / np.diag(Sigma) - 1.0).max()
    e2 = np.abs(np.diag(fc["covs"][-1]) / np.diag(Sigma) - 1.0).max()
    print(e1, e2)
    assert max(e1, e2) <= 1e-8, (e1, e2)


@pytest.mark.parametrize("model", ["rbc", "full_nk"])
def test_one_step_forecast_is_the_filters_prediction(model):
    """From the oracle filter's stored (a_filt[t], P_filt[t]) one forecast step gives its (a_pred[t+1], P_pred[t+1]).  Conventions:
    ``oracle.DEFAULT_CONVENTIONS`` (jitter on F and on P+, Joseph form) -- the stored P_filt already carries its jitter, so the
    identity holds on the stored outputs under every ``FilterConventions``; the defaults and the jitter-free variant are run."""
    T, R = _model(model)
    m, k = R.shape
    q = np.linspace(0.5, 1.5, k) * 1e-4
    Z = np.zeros((2, m))
    Z[0, 0], Z[1, m - 1] = 1.0, 1.0
    y = np.random.default_rng(5).normal(0, 0.02, (6, 2))
    for cv in (oracle.DEFAULT_CONVENTIONS, oracle.FilterConventions(jitter_on_P=False, joseph=False)):
        _, _, st = oracle.kalman_filter_logp(y, T, R, np.diag(q), Z, H=1e-6 * np.eye(2), return_states=True, conventions=cv)
        for t in range(5):
            fc = dr.forecast(T, R, q, st["a_filt"][t], st["P_filt"][t], 1)
            assert np.abs(fc["states"][0] - st["a_pred"][t + 1]).max() <= 1e-15 * max(1.0, np.abs(st["a_pred"]).max())
            assert np.abs(fc["covs"][0] - st["P_pred"][t + 1]).max() <= 1e-14 * np.abs(st["P_pred"]).max()


def test_wrapper_shape_checks():
    T, R = np.zeros((2, 4, 4)), np.zeros((2, 4, 3))
    eps = np.zeros((5, 6, 3))
    # simulate
    for bad in (dict(T=T[:, :3]), dict(R=np.zeros((2, 3, 3))), dict(eps=np.zeros((5, 6, 2))), dict(eps=np.zeros((3, 5, 6, 3))),
                dict(eps=np.zeros((6, 3))), dict(n_steps=5), dict(x0=np.zeros((5, 3))), dict(x0=np.zeros((3, 5, 4))),
                dict(status=np.zeros(3, dtype=np.int32)), dict(T=np.zeros((2, 97, 97)), R=np.zeros((2, 97, 3)))):
        with pytest.raises(ValueError):
            batched.simulate_batched(**{**dict(T=T, R=R, eps=eps), **bad})
    # impulse responses
    for bad in (dict(T=T[:, :3]), dict(S=np.zeros((4, 2))), dict(S=np.zeros((3, 3, 2))), dict(S=np.zeros(3)),
                dict(weights=np.ones(2)), dict(S=np.zeros((3, 5)), weights=np.ones(3)), dict(irf=False), dict(n_steps=-1),
                dict(status=np.zeros((2, 1), dtype=np.int32))):
        with pytest.raises(ValueError):
            batched.impulse_response_batched(**{**dict(T=T, R=R), **bad})
    # forecast
    a0 = np.zeros((2, 4))
    for bad in (dict(T=T[:, :3]), dict(a0=np.zeros((2, 3))), dict(P0=np.zeros((2, 4, 3))), dict(Q=np.ones(2), q_mode="diag"),
                dict(covariances="both"), dict(Z=np.zeros((2, 3))), dict(d=np.zeros(2)), dict(Z=np.zeros((2, 4)), Hdiag=np.zeros(3)),
                dict(n_steps=-1), dict(status=np.zeros(1, dtype=np.int32))):
        with pytest.raises(ValueError):
            batched.forecast_batched(**{**dict(T=T, R=R, Q=np.ones(3), a0=a0), **bad})
