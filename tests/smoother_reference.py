"""Numpy references of the fixed-interval smoother (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

``rts_smoother`` restates the recursion pymc_extras runs on the filter's outputs (Rauch-Tung-Striebel with
``pinv(P_pred, hermitian=True)``; unpinned like the rest of the filter half, oracle/statespace.py) plus the smoothed shocks
``eps[t+1] = Q R' P_pred[t+1]^+ (as[t+1] - a_pred[t+1])``; ``brute_force_smoother`` conditions the joint Gaussian of the
pre-sample state and all shocks on the data, without any recursion."""
import numpy as np
import scipy.linalg as sla


def rts_smoother(states, T, R, Q):
    """``states``: the dict of ``oracle.kalman_filter_logp(..., return_states=True)``.  Returns (smoothed states (n, m),
    smoothed covariances (n, m, m), smoothed shocks (n, k) with row 0 = NaN)."""
    a_pred, P_pred, a_filt, P_filt = (states[x] for x in ("a_pred", "P_pred", "a_filt", "P_filt"))
    n, m = a_filt.shape
    k = R.shape[1]
    a_s = np.empty((n, m))
    V = np.empty((n, m, m))
    eps = np.full((n, k), np.nan)
    a_s[-1], V[-1] = a_filt[-1], P_filt[-1]
    for t in range(n - 2, -1, -1):
        Pp = P_pred[t + 1]
        Pinv = np.linalg.pinv(Pp, hermitian=True)
        w = Pinv @ (a_s[t + 1] - a_pred[t + 1])
        a_s[t] = a_filt[t] + P_filt[t] @ (T.T @ w)
        eps[t + 1] = Q @ (R.T @ w)
        G = P_filt[t] @ T.T @ Pinv
        S = G @ (V[t + 1] - Pp) @ G.T
        V[t] = P_filt[t] + 0.5 * (S + S.T)
    return a_s, V, eps


def range_smoother(states, T, R, Q, rank_tol=1e-10):
    """The DEVICE's form of the same recursion (csrc/dsge_kalman_smooth.hpp), restated: the pseudo-inverse of P_pred from its
    range, which is fixed per draw.  U (m x r) is an orthonormal basis of [T | R_J], J = {j : Q_jj > 0}, by column-pivoted QR with
    the rank |R_jj| > rank_tol |R_00|; per step M = sym(U' P_pred U) and P_pred^+ x = U M^-1 U' x; everything else as in
    ``rts_smoother``.  Returns (smoothed states, covariances, shocks, r, min over the steps of lambda_min(M) / lambda_max(M))."""
    a_pred, P_pred, a_filt, P_filt = (states[x] for x in ("a_pred", "P_pred", "a_filt", "P_filt"))
    n, m = a_filt.shape
    k = R.shape[1]
    J = np.diag(Q) > 0
    Qf, Rf, _ = sla.qr(np.hstack([T, R[:, J]]), mode="economic", pivoting=True)
    dg = np.abs(np.diag(Rf))
    r = int(np.count_nonzero(dg > rank_tol * dg[0]))
    U = Qf[:, :r]
    a_s = np.empty((n, m))
    V = np.empty((n, m, m))
    eps = np.full((n, k), np.nan)
    a_s[-1], V[-1] = a_filt[-1], P_filt[-1]
    lam = np.inf
    for t in range(n - 2, -1, -1):
        Pp = P_pred[t + 1]
        M = U.T @ Pp @ U
        M = 0.5 * (M + M.T)
        ev = np.linalg.eigvalsh(M)
        lam = min(lam, ev[0] / ev[-1])
        w = U @ np.linalg.solve(M, U.T @ (a_s[t + 1] - a_pred[t + 1]))
        a_s[t] = a_filt[t] + P_filt[t] @ (T.T @ w)
        eps[t + 1] = Q @ (R.T @ w)
        G = (U @ np.linalg.solve(M, U.T @ T @ P_filt[t])).T  # P_filt T' U M^-1 U'  (P_filt, M symmetric)
        S = G @ (V[t + 1] - Pp) @ G.T
        V[t] = P_filt[t] + 0.5 * (S + S.T)
    return a_s, V, eps, r, lam


def brute_force_smoother(y, T, R, Q, Z, H, jitter_F, missing_fill_value=-9999.0):
    """E[x_t | y], Cov[x_t | y], E[eps_t | y] by conditioning u = [x_{-1}, eps_0 .. eps_{n-1}] ~ N(0, blockdiag(dlyap(T, R Q R'),
    Q, ..., Q)) on the observed entries of y_t = Z x_t + noise, noise ~ N(0, H + jitter_F I), with x_t = T x_{t-1} + R eps_t."""
    y = np.asarray(y, dtype=np.float64)
    n, p = y.shape
    m, k = R.shape
    P0 = sla.solve_discrete_lyapunov(T, R @ Q @ R.T)
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
    rows, vals, noise = [], [], []
    Hn = np.asarray(H, dtype=np.float64) + jitter_F * np.eye(p)
    for t in range(n):
        obs = ~(np.isnan(y[t]) | (y[t] == missing_fill_value))
        for o in np.flatnonzero(obs):
            rows.append(Z[o] @ L[t])
            vals.append(y[t, o])
            noise.append((t, o))
    Aobs = np.array(rows)
    N = np.zeros((len(rows), len(rows)))
    for i, (t, o) in enumerate(noise):
        for j, (t2, o2) in enumerate(noise):
            if t == t2:
                N[i, j] = Hn[o, o2]
    S = Aobs @ Su @ Aobs.T + N
    K = np.linalg.solve(S, Aobs @ Su).T  # Su Aobs' S^-1
    u_mean = K @ np.array(vals)
    u_cov = Su - K @ Aobs @ Su
    a_s = np.array([L[t] @ u_mean for t in range(n)])
    V = np.array([L[t] @ u_cov @ L[t].T for t in range(n)])
    eps = u_mean[m:].reshape(n, k)
    return a_s, V, eps
