"""Numpy reference of the simulation smoother (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

``simulation_smoother`` restates the draw of include/dsge_hip.h (``dsge_simulation_smoother_batched``) for ONE parameter draw and
ONE path in oracle terms: simulate x+, form y*, filter it with ``oracle.kalman_filter_logp`` under the call's d and conventions,
smooth with ``tests.smoother_reference.rts_smoother``, add x+ and eps+ back.  ``joint_conditional`` conditions the joint Gaussian
of the pre-sample state and all shocks on the data without any recursion and returns the JOINT moments over all time pairs."""
import numpy as np

import oracle

from tests.smoother_reference import rts_smoother


def simulation_smoother(y, T, R, Q, Z, H, d, x0, eps, eta, conventions=None, missing_fill_value=-9999.0):
    """y (n, p); H (p, p); d (p,) or None; x0 (m,) or None; eps (n, k); eta (n, p) or None.  Returns (x~ (n, m), eps~ (n, k)
    with row 0 = NaN)."""
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape[0], T.shape[0]
    xp = np.empty((n, m))
    x = np.zeros(m) if x0 is None else np.asarray(x0, dtype=np.float64)
    for t in range(n):
        x = T @ x + R @ eps[t]
        xp[t] = x
    miss = np.isnan(y) | (y == missing_fill_value)
    ystar = y - xp @ Z.T - (0.0 if eta is None else eta)
    ystar[miss] = y[miss]  # a missing entry stays missing
    _, _, stt = oracle.kalman_filter_logp(ystar, T, R, Q, Z, H=H, d=d, return_states=True, conventions=conventions,
                                          missing_fill_value=missing_fill_value)
    a_s, _, e_s = rts_smoother(stt, T, R, Q)
    return xp + a_s, eps + e_s


def joint_conditional(y, T, R, Q, Z, H, jitter_F, missing_fill_value=-9999.0):
    """Mean and JOINT covariance of the stacked states [x_0 .. x_{n-1}] (n m) and of the stacked shocks [eps_1 .. eps_{n-1}]
    ((n - 1) k) given the observed entries of y_t = Z x_t + noise, noise ~ N(0, H + jitter_F I), by conditioning
    u = [x_{-1}, eps_0 .. eps_{n-1}] ~ N(0, blockdiag(dlyap(T, R Q R'), Q, ..., Q)).  Returns (x mean (n, m), x cov (n m, n m),
    eps mean (n - 1, k), eps cov ((n - 1) k, (n - 1) k), P0)."""
    y = np.asarray(y, dtype=np.float64)
    n, p = y.shape
    m, k = R.shape
    P0 = oracle.solve_discrete_lyapunov(T, R @ Q @ R.T)
    nu = m + n * k
    Su = np.zeros((nu, nu))
    Su[:m, :m] = P0
    for t in range(n):
        Su[m + t * k:m + (t + 1) * k, m + t * k:m + (t + 1) * k] = Q
    L = np.zeros((n, m, nu))  # x_t = L[t] u
    prev = np.zeros((m, nu))
    prev[:, :m] = np.eye(m)
    for t in range(n):
        cur = T @ prev
        cur[:, m + t * k:m + (t + 1) * k] += R
        L[t] = cur
        prev = cur
    Hn = np.asarray(H, dtype=np.float64) + jitter_F * np.eye(p)
    rows, vals, where = [], [], []
    for t in range(n):
        for o in np.flatnonzero(~(np.isnan(y[t]) | (y[t] == missing_fill_value))):
            rows.append(Z[o] @ L[t])
            vals.append(y[t, o])
            where.append((t, o))
    A = np.array(rows)
    N = np.array([[Hn[o, o2] if t == t2 else 0.0 for (t2, o2) in where] for (t, o) in where])
    S = A @ Su @ A.T + N
    K = np.linalg.solve(S, A @ Su).T
    u_mean = K @ np.array(vals)
    u_cov = Su - K @ A @ Su
    Lx = L.reshape(n * m, nu)
    return ((Lx @ u_mean).reshape(n, m), Lx @ u_cov @ Lx.T, u_mean[m + k:].reshape(n - 1, k), u_cov[m + k:, m + k:], P0)
