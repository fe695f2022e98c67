"""Numpy references of the smoother across dated structural breaks (TEST INFRASTRUCTURE ONLY; a helper, not a test module), one draw
(docs/design/segmented_smoother.md).

``segmented_forward`` writes the forward chain of tests/segmented_filter_reference.py out again, keeping the moments of every period
(that helper returns ``P_pred`` alone): ``oracle.kalman_filter_logp(a0=, P0=, return_states=True, conventions=)`` per segment and the
boundary step.  ``segmented_rts_smoother`` is the backward recursion with ``pinv(P_pred, hermitian=True)``; step t uses the matrices of
s' = s(t+1).  ``segmented_range_smoother`` restates the DEVICE's form: the pseudo-inverse from the range of ``[T_s' | R_s',J]``, one
basis per segment (modelled on ``range_smoother`` of tests/smoother_reference.py).  ``brute_force_segmented_smoother`` conditions
u = [x_0, eps_1 .. eps_{n-1}] on the data without any recursion."""
import numpy as np
import scipy.linalg as sla

import oracle

from tests.segmented_filter_reference import segment_of


def _sym(A):
    return 0.5 * (A + A.T)


def segmented_forward(y, segs, seg_start, a0=None, P0=None, shift=None, jitter=oracle.JITTER_DEFAULT,
                      missing_fill_value=oracle.MISSING_FILL, conventions=None):
    """``segs``, ``shift`` as ``segmented_filter`` takes them.  Returns dict(ll (n,), a_pred, a_filt (n, m), P_pred, P_filt (n, m, m)):
    a_pred[0] = a0 or 0, P_pred[0] = P0 or the stationary covariance of segment 0; a_pred[t] holds shift at a boundary."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    bounds = list(seg_start) + [y.shape[0]]
    a, P = a0, P0
    keys = ("a_pred", "a_filt", "P_pred", "P_filt")
    parts = {key: [] for key in ("ll", *keys)}
    for s, x in enumerate(segs):
        if s > 0:  # the boundary step, with the matrices of the segment being entered
            af = a if shift is None else a + np.asarray(shift)[s]
            a = x["T"] @ af
            P = _sym(x["T"] @ P @ x["T"].T) + _sym(x["R"] @ x["Q"] @ x["R"].T)
        _, ll_s, stt = oracle.kalman_filter_logp(y[bounds[s]:bounds[s + 1]], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], a0=a,
                                                 P0=P, jitter=jitter, missing_fill_value=missing_fill_value, return_states=True,
                                                 conventions=conventions)
        parts["ll"].append(ll_s)
        for key in keys:
            parts[key].append(stt[key])
        a, P = stt["a_filt"][-1], stt["P_filt"][-1]
    return {key: np.concatenate(v) for key, v in parts.items()}


def _backward(fwd, segs, seg_start, pinv_of):
    """The recursion of the issue; ``pinv_of(s, Pp)`` -> Pp^+ for a step that uses segment s."""
    a_pred, P_pred, a_filt, P_filt = (fwd[x] for x in ("a_pred", "P_pred", "a_filt", "P_filt"))
    n, m = a_filt.shape
    k = segs[0]["R"].shape[1]
    a_s, V, eps = np.empty((n, m)), np.empty((n, m, m)), np.full((n, k), np.nan)
    a_s[-1], V[-1] = a_filt[-1], P_filt[-1]
    for t in range(n - 2, -1, -1):
        x = segs[segment_of(seg_start, t + 1)]
        Pp = P_pred[t + 1]
        Pinv = pinv_of(segment_of(seg_start, t + 1), Pp)
        w = Pinv @ (a_s[t + 1] - a_pred[t + 1])
        a_s[t] = a_filt[t] + P_filt[t] @ (x["T"].T @ w)
        eps[t + 1] = x["Q"] @ (x["R"].T @ w)
        G = P_filt[t] @ x["T"].T @ Pinv
        V[t] = P_filt[t] + _sym(G @ (V[t + 1] - Pp) @ G.T)
    return a_s, V, eps


def segmented_rts_smoother(fwd, segs, seg_start):
    """(smoothed states (n, m), covariances (n, m, m), shocks (n, k) with row 0 = NaN) from the dict of ``segmented_forward``."""
    return _backward(fwd, segs, seg_start, lambda s, Pp: np.linalg.pinv(Pp, hermitian=True))


def segment_bases(segs, rank_tol=1e-10):
    """Per segment: an orthonormal basis U_s (m x r_s) of [T_s | R_s,J], J = {j : Q_s,jj > 0}, by column-pivoted QR with the rank
    |R_jj| > rank_tol |R_00|."""
    out = []
    for x in segs:
        J = np.diag(x["Q"]) > 0
        Qf, Rf, _ = sla.qr(np.hstack([x["T"], x["R"][:, J]]), mode="economic", pivoting=True)
        dg = np.abs(np.diag(Rf))
        out.append(Qf[:, :int(np.count_nonzero(dg > rank_tol * dg[0]))])
    return out


def segmented_range_smoother(fwd, segs, seg_start, rank_tol=1e-10):
    """The device's form: P_pred[t+1]^+ = U_s' M^-1 U_s'' with M = sym(U_s'' P_pred[t+1] U_s').  Returns (states, covariances,
    shocks, the ranks r_s)."""
    U = segment_bases(segs, rank_tol)

    def pinv_of(s, Pp):
        return U[s] @ np.linalg.solve(_sym(U[s].T @ Pp @ U[s]), U[s].T)

    return (*_backward(fwd, segs, seg_start, pinv_of), [u.shape[1] for u in U])


def brute_force_segmented_smoother(y, segs, seg_start, a0, P0, shift, jitter_F, missing_fill_value=oracle.MISSING_FILL):
    """E[x_t | y], Cov[x_t | y], E[eps_t | y] by conditioning u = [x_0, eps_1 .. eps_{n-1}], x_0 ~ N(a0, P0), eps_t ~ N(0, Q_s(t)),
    x_t = T_s(t) (x_{t-1} + [t == seg_start[s]] shift_s) + R_s(t) eps_t, on the observed entries of y_t = Z_s x_t + d_s + noise,
    noise ~ N(0, H_s + jitter_F I).  x_t = L_t u + c_t is written out; no recursion over moments.  Row 0 of the shocks is NaN."""
    y = np.asarray(y, dtype=np.float64)
    n, p = y.shape
    m, k = segs[0]["R"].shape
    nu = m + (n - 1) * k
    mu = np.zeros(nu)
    mu[:m] = a0
    Su = np.zeros((nu, nu))
    Su[:m, :m] = P0
    L, c = np.zeros((n, m, nu)), np.zeros((n, m))
    L[0, :, :m] = np.eye(m)
    for t in range(1, n):
        s = segment_of(seg_start, t)
        x = segs[s]
        sl = slice(m + (t - 1) * k, m + t * k)
        Su[sl, sl] = x["Q"]
        L[t] = x["T"] @ L[t - 1]
        L[t][:, sl] += x["R"]
        c[t] = x["T"] @ (c[t - 1] + (shift[s] if shift is not None and t == seg_start[s] else 0.0))
    rows, vals, where = [], [], []
    for t in range(n):
        x = segs[segment_of(seg_start, t)]
        d = np.zeros(p) if x["d"] is None else x["d"]
        for o in np.flatnonzero(~(np.isnan(y[t]) | (y[t] == missing_fill_value))):
            rows.append(x["Z"][o] @ L[t])
            vals.append(y[t, o] - d[o] - x["Z"][o] @ c[t])
            where.append((t, o))
    A = np.array(rows)
    N = np.zeros((len(rows), len(rows)))
    for i, (t, o) in enumerate(where):
        Hs = segs[segment_of(seg_start, t)]["H"]
        for j, (t2, o2) in enumerate(where):
            if t == t2:
                N[i, j] = (0.0 if Hs is None else Hs[o, o2]) + (jitter_F if o == o2 else 0.0)
    K = np.linalg.solve(A @ Su @ A.T + N, A @ Su).T
    u_mean = mu + K @ (np.array(vals) - A @ mu)
    u_cov = Su - K @ A @ Su
    a_s = np.array([L[t] @ u_mean + c[t] for t in range(n)])
    V = np.array([L[t] @ u_cov @ L[t].T for t in range(n)])
    eps = np.full((n, k), np.nan)
    eps[1:] = u_mean[m:].reshape(n - 1, k)
    return a_s, V, eps
