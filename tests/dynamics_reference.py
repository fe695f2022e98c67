"""Numpy references of the post-solve dynamics (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the propagation loop
``x_t = T x_{t-1} + R e_t``, the forecast-error variance decomposition from its definition and the forecast moment recursion
exactly as include/dsge_hip.h states it.  Written fresh; ``tests/golden/dynamics_reference.npz`` holds what the reference's
own loop gives on two models (tests/test_dynamics_reference.py compares)."""
import numpy as np


def propagate(T, R, eps, n_steps=None, x0=None):
    """``eps``: (n_shock_steps, k).  Returns x (n_steps, m) with x[-1] = x0 (zero by default) and no shock from step
    n_shock_steps on."""
    eps = np.asarray(eps, dtype=np.float64)
    n_steps = eps.shape[0] if n_steps is None else n_steps
    x = np.zeros(T.shape[0]) if x0 is None else np.asarray(x0, dtype=np.float64)
    out = np.empty((n_steps, T.shape[0]))
    for t in range(n_steps):
        x = T @ x
        if t < eps.shape[0]:
            x = x + R @ eps[t]
        out[t] = x
    return out


def impulse_responses(T, R, n_steps, S=None):
    """irf[j, h] = T^h R S[:, j]  ->  (c, n_steps, m); S = I_k by default."""
    S = np.eye(R.shape[1]) if S is None else np.asarray(S, dtype=np.float64)
    return np.stack([propagate(T, R, S[:, j][None, :], n_steps) for j in range(S.shape[1])])


def fevd_totals(irf, weights=None):
    """w_j sum_{s<=h} irf[j, s, i]^2  ->  (n_steps, m, c): the numerators of the decomposition."""
    c = irf.shape[0]
    w = np.ones(c) if weights is None else np.asarray(weights, dtype=np.float64)
    return np.transpose(np.cumsum(irf ** 2, axis=1) * w[:, None, None], (1, 2, 0))


def fevd(irf, weights=None):
    """fevd[h, i, j] = numerator / sum over j; a zero denominator gives NaN in that row."""
    num = fevd_totals(irf, weights)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / num.sum(axis=2, keepdims=True)


def forecast(T, R, Q, a0, P0, n_steps, Z=None, d=None, Hdiag=None):
    """a_h = T a_{h-1};  P_h = sym(T P_{h-1} T') + sym(R Q R');  y_h = Z a_h + d;  F_h = sym(Z P_h Z') + diag(H), h = 1..n_steps.
    ``Q``: (k,) variances or (k, k).  Returns dict(states, covs, observed, observed_covs) (the last two None without Z)."""
    m = T.shape[0]
    Q = np.diag(Q) if np.ndim(Q) == 1 else np.asarray(Q)
    G = R @ Q @ R.T
    G = 0.5 * (G + G.T)
    a = np.asarray(a0, dtype=np.float64)
    P = np.zeros((m, m)) if P0 is None else np.asarray(P0, dtype=np.float64)
    out = dict(states=np.empty((n_steps, m)), covs=np.empty((n_steps, m, m)), observed=None, observed_covs=None)
    if Z is not None:
        p = Z.shape[0]
        d = np.zeros(p) if d is None else d
        Hdiag = np.zeros(p) if Hdiag is None else Hdiag
        out["observed"], out["observed_covs"] = np.empty((n_steps, p)), np.empty((n_steps, p, p))
    for h in range(n_steps):
        a = T @ a
        TPT = T @ P @ T.T
        P = 0.5 * (TPT + TPT.T) + G
        out["states"][h], out["covs"][h] = a, P
        if Z is not None:
            ZPZ = Z @ P @ Z.T
            out["observed"][h] = Z @ a + d
            out["observed_covs"][h] = 0.5 * (ZPZ + ZPZ.T) + np.diag(Hdiag)
    return out
