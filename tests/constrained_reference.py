"""Numpy reference of the perfect-foresight paths under an occasionally binding bound (TEST INFRASTRUCTURE ONLY; a helper, not a
test module): one draw, one path.

The model, ``T``, ``R``, ``M = B + C T`` and ``G`` are those of tests/anticipated_reference.py.  A row ``c``, a ``bound``, a shock
column ``s`` and a horizon ``H``: shadow shocks ``nu[0 .. H-1] >= 0``, known at t = 0 like ``eps``, are added to column ``s`` so that
    x[t] = T x[t-1] + w[t],   w[t] = G w[t+1] + R (eps[t] + nu[t] e_s),   gap[t] = c'x[t] - bound,
    gap[h] >= 0,  nu[h] >= 0,  nu[h] gap[h] = 0   for h < H   (Holden and Paetz).
``Mz[h][j] = c'x[h]`` of the path from ``x0 = 0`` with a unit shock on column ``s`` at period ``j`` alone, ``q[h] = c'xu[h] - bound``
on the unconstrained path ``xu``; ``gap = q + Mz nu`` on ``h < H``.  The regime iteration: ``S = {q < 0}``; solve
``Mz[S, S] nu[S] = -q[S]`` (``np.linalg.solve``), ``nu = 0`` off ``S``, ``gap = q + Mz nu``,
``S' = {h in S : nu[h] > 0} | {h not in S : gap[h] < 0}``, until ``S' == S``; every comparison strict, no tolerance.
tests/test_constrained_reference.py holds it to independent formulations."""
import numpy as np

from tests import anticipated_reference as ref

NO_REGIME, SINGULAR, BEYOND_HORIZON, SKIPPED = 1, 2, 4, 8
BEYOND_TOL = 1e-12


def pad_shocks(eps, H):
    """eps (n_shock, k) with zero rows up to max(n_shock, H)."""
    out = np.zeros((max(eps.shape[0], H), eps.shape[1]))
    out[:eps.shape[0]] = eps
    return out


def shadow_matrix(G, T, R, c, s, H):
    """Mz (H, H)."""
    k = R.shape[1]
    Mz = np.empty((H, H))
    for j in range(H):
        e = np.zeros((H, k))
        e[j, s] = 1.0
        Mz[:, j] = ref.propagate(T, ref.anticipation(G, R, e, H, "perfect_foresight")) @ c
    return Mz


def pivots(A):
    """The pivots of the row-pivoted elimination of A, in the order of its columns."""
    A = np.array(A, dtype=np.float64)
    out = []
    for j in range(A.shape[0]):
        r = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, r]] = A[[r, j]]
        out.append(A[j, j])
        if A[j, j] != 0.0 and np.isfinite(A[j, j]):
            A[j + 1:] -= np.outer(A[j + 1:, j] / A[j, j], A[j])
    return np.array(out)


def regime_iteration(Mz, q, max_iter=0, rank_tol=0.0):
    """dict(nu (H,), S (H,) bool, iters, status, margin): ``margin`` is the smallest |decision quantity| -- q at the start, nu on S
    and gap off S afterwards -- over the iterations."""
    H = q.shape[0]
    max_iter = max_iter if max_iter > 0 else 64
    thr = (rank_tol if rank_tol > 0.0 else 1e-14) * np.abs(Mz).max()
    nu = np.zeros(H)
    if not np.isfinite(q).all():
        return dict(nu=nu, S=np.zeros(H, bool), iters=0, status=SINGULAR, margin=0.0)
    S = q < 0.0
    margin = np.abs(q).min()
    iters = 0
    while True:
        iters += 1
        nu = np.zeros(H)
        if S.any():
            K = Mz[np.ix_(S, S)]
            piv = pivots(K)
            if not (np.abs(piv) > thr).all():
                return dict(nu=nu, S=S, iters=iters, status=SINGULAR, margin=margin)
            nu[S] = np.linalg.solve(K, -q[S])
        gap = q + Mz @ nu
        margin = min(margin, np.abs(np.where(S, nu, gap)).min())
        S_new = np.where(S, nu > 0.0, gap < 0.0)
        if (S_new == S).all():
            return dict(nu=nu, S=S, iters=iters, status=0, margin=margin)
        if iters >= max_iter:
            return dict(nu=nu, S=S, iters=iters, status=NO_REGIME, margin=margin)
        S = S_new


def constrained_paths(B, C, T, R, eps, c, bound, s, H, n_steps, x0=None, Z=None, d=None, max_iter=0, rank_tol=0.0):
    """dict(x, w (n_steps, n), observed (n_steps, p) or None, nu (H,), gap (n_steps,), Mz (H, H), q (H,), S, iters, status, margin,
    G, M) of one draw and path; NaN in x, w, observed, nu and gap of a path without a regime or with a singular system."""
    G, M = ref.gain(B, C, T)
    Mz = shadow_matrix(G, T, R, c, s, H)
    xu = ref.propagate(T, ref.anticipation(G, R, eps, n_steps, "perfect_foresight"), x0)
    q = xu[:H] @ c - bound
    it = regime_iteration(Mz, q, max_iter, rank_tol)
    e = pad_shocks(eps, H)
    e[:H, s] += it["nu"]
    r = ref.anticipated_paths(B, C, T, R, e, n_steps, "perfect_foresight", x0, Z, d)
    gap = r["x"] @ c - bound
    status = it["status"]
    out = dict(x=r["x"], w=r["w"], observed=r["observed"], nu=it["nu"], gap=gap)
    if status & (NO_REGIME | SINGULAR):
        out = {key: None if a is None else np.full_like(a, np.nan) for key, a in out.items()}
    elif (gap[H:] < -BEYOND_TOL * np.abs(q).max()).any():
        status |= BEYOND_HORIZON
    return dict(out, Mz=Mz, q=q, S=it["S"], iters=it["iters"], status=status, margin=it["margin"], G=G, M=M, xu=xu)
