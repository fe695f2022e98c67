"""Numpy reference of the stochastic simulation at an occasionally binding bound (TEST INFRASTRUCTURE ONLY; a helper, not a test
module): one draw, one path, written by the definition and NOT through the tables ``Cq = c'T^h`` and ``W = G^j R[:, s]`` of the
device kernels.

The model, ``Mz`` and the regime iteration are those of tests/constrained_reference.py.  ``eps[t]`` is a surprise at ``t``; every
period:
    xu   = the unconstrained H-period path from x[t-1] with eps[t] at its period 0 and no shock afterwards   (``aref.propagate``)
    q    = xu c - bound
    nu   = ``ref.regime_iteration(Mz, q)``                                                                   (the plan of period t)
    x[t] = period 0 of ``aref.anticipated_paths`` from x[t-1] on the shocks eps[t] at period 0 plus nu on column s.
Only ``nu[0]`` is realised; the plan is revised next period.  tests/test_constrained_sim_reference.py holds it to independent
formulations."""
import numpy as np

from tests import anticipated_reference as aref
from tests import constrained_reference as ref

NO_REGIME, SINGULAR, SKIPPED, HORIZON_SHORT = ref.NO_REGIME, ref.SINGULAR, ref.SKIPPED, 16


def constrained_simulate(B, C, T, R, eps, c, bound, s, H, n_steps, x0=None, Z=None, d=None, max_iter=0, rank_tol=0.0):
    """dict(x (n_steps, n), observed (n_steps, p) or None, gap, shadow (n_steps,), plan (n_steps, H), duration, iters (n_steps,)
    int, status, fail_step, margin, Mz (H, H), q (n_steps, H), S (n_steps, H) bool, qmax (n_steps,), G, M) of one draw and path.
    ``margin``: the smallest over periods of ``regime_iteration``'s margin divided by that period's max|q|.  A path that fails in
    period f keeps the periods before f and has NaN from f on (iters: the count at f, then 0; duration: -1)."""
    n, k = R.shape
    G, M = aref.gain(B, C, T)
    Mz = ref.shadow_matrix(G, T, R, c, s, H)
    p = 0 if Z is None else Z.shape[0]
    x, obs = np.full((n_steps, n), np.nan), (None if Z is None else np.full((n_steps, p), np.nan))
    gap, shadow, plan = np.full(n_steps, np.nan), np.full(n_steps, np.nan), np.full((n_steps, H), np.nan)
    duration, iters = np.full(n_steps, -1, np.int32), np.zeros(n_steps, np.int32)
    q_all, S_all, qmax = np.full((n_steps, H), np.nan), np.zeros((n_steps, H), bool), np.full(n_steps, np.nan)
    prev = np.zeros(n) if x0 is None else np.asarray(x0, dtype=np.float64)
    status, fail_step, margin = 0, -1, np.inf
    for t in range(n_steps):
        e = np.zeros((H, k))
        if t < eps.shape[0]:
            e[0] = eps[t]
        w = np.zeros((H, n))
        w[0] = R @ e[0]
        q = aref.propagate(T, w, prev) @ c - bound
        it = ref.regime_iteration(Mz, q, max_iter, rank_tol)
        q_all[t], iters[t] = q, it["iters"]
        if it["status"]:
            status |= it["status"]
            fail_step = t
            break
        qmax[t], S_all[t] = np.abs(q).max(), it["S"]
        margin = min(margin, it["margin"] / qmax[t])
        e[:, s] += it["nu"]
        prev = aref.anticipated_paths(B, C, T, R, e, H, "perfect_foresight", prev)["x"][0]
        x[t], plan[t], shadow[t], duration[t] = prev, it["nu"], it["nu"][0], int(it["S"].sum())
        gap[t] = prev @ c - bound
        if Z is not None:
            obs[t] = Z @ prev + (0.0 if d is None else d)
        if it["S"][H - 1]:
            status |= HORIZON_SHORT
    return dict(x=x, observed=obs, gap=gap, shadow=shadow, plan=plan, duration=duration, iters=iters, status=status,
                fail_step=fail_step, margin=margin, Mz=Mz, q=q_all, S=S_all, qmax=qmax, G=G, M=M)


def tables(G, T, R, c, s, H):
    """(Cq (H, n), W (n, H)): Cq[h] = c'T^h, W[:, j] = G^j R[:, s] -- the per-draw tables of the device kernels."""
    Cq, W = np.empty((H, T.shape[0])), np.empty((T.shape[0], H))
    row, col = c.astype(np.float64), R[:, s].copy()
    for h in range(H):
        Cq[h], W[:, h] = row, col
        row, col = row @ T, G @ col
    return Cq, W
