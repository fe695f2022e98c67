"""Numpy reference of the conditional forecast (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the hard conditions of
Waggoner and Zha (1999) with the matrix W written out from matrix powers and ``np.linalg.solve`` -- nothing of the device's
Toeplitz sums, tile order or Cholesky factor.  One draw, one path per call; float64."""
import numpy as np


def simulate(T, R, e, x0):
    """x[t] = T x[t-1] + R e[t], t = 0 .. len(e)-1, x[-1] = x0."""
    x, out = np.asarray(x0, dtype=float), np.empty((len(e), T.shape[0]))
    for t in range(len(e)):
        x = T @ x + R @ e[t]
        out[t] = x
    return out


def system(T, R, Q, Z, cond_t, cond_j, free):
    """(W (n_cond, (t_max + 1) |F|), Qt = I (x) Q_FF) of the conditions, from matrix powers."""
    F = np.asarray(free, dtype=int)
    nF, t_max = len(F), int(max(cond_t))
    W = np.zeros((len(cond_t), (t_max + 1) * nF))
    for c, (t, j) in enumerate(zip(cond_t, cond_j)):
        for s in range(t + 1):
            W[c, s * nF:(s + 1) * nF] = (Z[j] @ np.linalg.matrix_power(T, t - s) @ R)[F]
    return W, np.kron(np.eye(t_max + 1), Q[np.ix_(F, F)])


def conditional_forecast(T, R, Q, Z, d, x0, cond_t, cond_j, cond_val, n_steps, eps=None, free=None, WQ=None):
    """dict(x (n_steps, m), shocks (n_steps, k), observed (n_steps, p), G).  Q: (k, k); d: (p,) or None; eps: (n_shock_steps, k) or
    None; free: the indices of the free shocks, default all; WQ: ``system(...)`` of the same draw, when the caller has it."""
    m, k = R.shape
    d = np.zeros(Z.shape[0]) if d is None else np.asarray(d, dtype=float)
    e = np.zeros((n_steps, k))
    if eps is not None:
        e[:len(eps)] = eps
    G = None
    if len(cond_t):
        F = np.arange(k) if free is None else np.asarray(sorted(free), dtype=int)
        W, Qt = WQ if WQ is not None else system(T, R, Q, Z, cond_t, cond_j, F)
        xb = simulate(T, R, e, x0)
        r = np.array([v - d[j] - Z[j] @ xb[t] for t, j, v in zip(cond_t, cond_j, cond_val)])
        G = W @ Qt @ W.T
        delta = (Qt @ W.T @ np.linalg.solve(G, r)).reshape(-1, len(F))
        e[:delta.shape[0], F] += delta
    x = simulate(T, R, e, x0)
    return dict(x=x, shocks=e, observed=x @ Z.T + d, G=G)
