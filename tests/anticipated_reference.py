"""Numpy reference of the anticipated-shock paths (TEST INFRASTRUCTURE ONLY; a helper, not a test module): one draw, one path.

The model is ``A x[t-1] + B x[t] + C E_t x[t+1] + D eps[t] = 0`` with the solution ``T``; ``M = B + C T``, ``G = -M^-1 C`` by
``np.linalg.solve``, ``R = -M^-1 D``.  Then ``x[t] = T x[t-1] + w[t]``, ``x[-1] = x0``, with
  perfect foresight:  ``w[S] = 0``, ``w[t] = G w[t+1] + R eps[t]``            (eps (S, k), the whole path known at t = 0)
  news:               ``w[t] = R e[t][0] + G (R e[t][1] + G (... R e[t][L]))``  (e (S, L + 1, k), e[t][j] = E_t eps[t+j])
tests/test_anticipated_reference.py holds it to independent formulations."""
import numpy as np


def gain(B, C, T):
    """(G, M) of one draw."""
    M = B + C @ T
    return np.linalg.solve(M, -C), M


def anticipation(G, R, eps, n_steps, mode):
    """w (n_steps, n): the anticipation term of one path."""
    n = G.shape[0]
    n_shock = eps.shape[0]
    W = np.zeros((max(n_shock, n_steps), n))
    if mode == "perfect_foresight":
        w = np.zeros(n)
        for t in range(n_shock - 1, -1, -1):
            w = G @ w + R @ eps[t]
            W[t] = w
    elif mode == "news":
        if n_shock > n_steps:
            raise ValueError("news: n_shock_steps > n_steps")
        for t in range(n_shock):
            acc = np.zeros(n)
            for j in range(eps.shape[1] - 1, -1, -1):
                acc = G @ acc + R @ eps[t, j]
            W[t] = acc
    else:
        raise ValueError(mode)
    return W[:n_steps]


def propagate(T, W, x0=None):
    """x (n_steps, n) with x[t] = T x[t-1] + W[t], x[-1] = x0 (zero by default)."""
    x = np.empty_like(W)
    prev = np.zeros(T.shape[0]) if x0 is None else x0
    for t in range(W.shape[0]):
        prev = T @ prev + W[t]
        x[t] = prev
    return x


def anticipated_paths(B, C, T, R, eps, n_steps, mode="perfect_foresight", x0=None, Z=None, d=None):
    """dict(x, w (n_steps, n), observed (n_steps, p) or None, G, M) of one draw and path."""
    G, M = gain(B, C, T)
    w = anticipation(G, R, eps, n_steps, mode)
    x = propagate(T, w, x0)
    obs = None if Z is None else x @ Z.T + (0.0 if d is None else d)
    return dict(x=x, w=w, observed=obs, G=G, M=M)


def triple_loop_expected_shocks(nu):
    """e[t][j] = sum_{i = 0 .. min(t, L - j)} nu[t - i][j + i] for nu (S, L + 1, k), by the definition."""
    S, L1, _ = nu.shape
    e = np.zeros_like(nu)
    for t in range(S):
        for j in range(L1):
            for i in range(min(t, L1 - 1 - j) + 1):
                e[t, j] += nu[t - i, j + i]
    return e
