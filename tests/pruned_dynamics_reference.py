"""Numpy restatement of the second-order dynamics (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the pruned recursion

    x_f' = T x_f + R u
    x_s' = T x_s + 1/2 g_yy (f (x) f) + g_yu (f (x) u) + 1/2 g_uu (u (x) u) + 1/2 g_ss,      f = x_f[S],      x = x_f + x_s

on the REDUCED solution ``sol = dict(g_yy (n, s, s), g_yu (n, s, k), g_uu (n, k, k), g_ss (n,), S)`` in the time indexing of
``dsge_simulate_batched`` (output index t holds the state after shock t), and the generalised impulse response from its definition.
Written with ``einsum`` on the unfolded blocks, not in the device's packed order; tests/test_pruned_dynamics_reference.py compares
it with ``oracle.second_order.simulate_pruned``.  Also the inputs the CPU and the GPU tests share."""
import functools

import numpy as np

from geconpy_amd import workloads as wl
from oracle import second_order as so


def simulate_pruned(T, R, sol, eps, n_steps=None, x0=None):
    """``eps``: (n_shock_steps, k), one path.  ``x0``: None or the pair (xf0, xs0).  -> (x_f, x_s), each (n_steps, n); steps from
    n_shock_steps on carry no shock."""
    n, k = R.shape
    S = np.asarray(sol["S"])
    eps = np.zeros((0, k)) if eps is None else np.asarray(eps, dtype=np.float64)
    n_steps = eps.shape[0] if n_steps is None else n_steps
    xf, xs = (np.zeros(n), np.zeros(n)) if x0 is None else (np.asarray(x0[0], dtype=np.float64), np.asarray(x0[1], dtype=np.float64))
    out_f, out_s = np.empty((n_steps, n)), np.empty((n_steps, n))
    for t in range(n_steps):
        u = eps[t] if t < eps.shape[0] else np.zeros(k)
        f = xf[S]
        quad = (0.5 * np.einsum("iab,a,b->i", sol["g_yy"], f, f) + np.einsum("iaj,a,j->i", sol["g_yu"], f, u)
                + 0.5 * np.einsum("ijl,j,l->i", sol["g_uu"], u, u) + 0.5 * sol["g_ss"])
        xs = T @ xs + quad
        xf = T @ xf + R @ u
        out_f[t], out_s[t] = xf, xs
    return out_f, out_s


def girf_pruned(T, R, sol, n_steps, impulses=None, eps=None, x0=None):
    """``impulses``: (k, c), default I_k.  ``eps``: None (one baseline path without shocks) or (n_paths, n_shock_steps, k); ``x0``: None
    or a pair of (n_paths, n).  -> (girf_f, girf_s), each (c, n_steps, n): the means over the baseline paths, in ascending order, of
    the differences between the path with ``e_0 += impulses[:, j]`` and the path itself, for the two parts."""
    n, k = R.shape
    imp = np.eye(k) if impulses is None else np.asarray(impulses, dtype=np.float64)
    base = np.zeros((1, 0, k)) if eps is None else np.asarray(eps, dtype=np.float64)
    n_paths = base.shape[0]
    out_f, out_s = np.zeros((imp.shape[1], n_steps, n)), np.zeros((imp.shape[1], n_steps, n))
    for j in range(imp.shape[1]):
        for p in range(n_paths):
            start = None if x0 is None else (x0[0][p], x0[1][p])
            shocked = np.zeros((max(base.shape[1], 1), k))
            shocked[:base.shape[1]] = base[p]
            shocked[0] += imp[:, j]
            bf, bs = simulate_pruned(T, R, sol, base[p], n_steps, start)
            sf, ss = simulate_pruned(T, R, sol, shocked, n_steps, start) if n_steps else (bf, bs)
            out_f[j] += sf - bf
            out_s[j] += ss - bs
    return out_f / n_paths, out_s / n_paths


def full_layout(sol, n):
    """The reduced solution scattered into the n^2 layout ``oracle.second_order.simulate_pruned`` takes."""
    S = np.asarray(sol["S"])
    k = sol["g_uu"].shape[-1]
    g_yy, g_yu = np.zeros((n, n, n)), np.zeros((n, n, k))
    g_yy[np.ix_(np.arange(n), S, S)] = sol["g_yy"]
    g_yu[:, S, :] = sol["g_yu"]
    return dict(g_yy=g_yy.reshape(n, n * n), g_yu=g_yu.reshape(n, n * k), g_uu=sol["g_uu"].reshape(n, k * k), g_ss=sol["g_ss"])


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
SHAPES = {  # name -> (n, s, n_lead, k); seeds as tests/test_gpu_second_order.py::_small_batch(n, s, n_lead, k, nb, 3100 + n)
    "n6": (6, 3, 2, 2),
    "n17": (17, 5, 4, 3),
    "n40": (40, 18, 12, 7),
    "n64": (64, 24, 16, 12),
    "n20": (20, 3, 6, 5),
}
PERMUTED = ("n17",)  # the state variables are NOT the first s ones: the variables are renumbered


@functools.lru_cache(maxsize=None)
def case(name, nb=3):
    """dict(T, R, g_yy, g_yu, g_uu, g_ss (leading draw axis), S, sigma (nb, k)) of ``nb`` draws of a SW-shaped system with a
    synthetic Hessian, solved by ``oracle.second_order.second_order_solution_reduced``; computed once, read-only."""
    n, s, nl, k = SHAPES[name]
    seed = 3100 + n
    sysm = [wl.sw_shaped_system(seed + i, n=n, n_state=s, n_lead=nl, k=k) for i in range(nb)]
    idx = wl.second_order_hessian_pattern(sysm[0][0], sysm[0][2], k, nnz_per_eq=6, seed=seed)
    val = np.random.default_rng(seed + 99).standard_normal((nb, len(idx)))
    sigma = np.random.default_rng(seed + 7).uniform(0.007, 0.02, (nb, k))
    S = np.arange(s)
    perm = np.arange(n)
    if name in PERMUTED:  # new variable perm[i] is old variable i; the states land on scattered, ascending positions
        perm = np.random.default_rng(seed + 5).permutation(n)
    out = {key: [] for key in ("T", "R", "g_yy", "g_yu", "g_uu", "g_ss")}
    order = np.argsort(perm[:s])  # old state a = S_old[a] sits at new position perm[a]; ascending new positions
    for i, (A, B, C, D, T) in enumerate(sysm):
        R = np.linalg.solve(B + C @ T, -D)
        sol = so.second_order_solution_reduced(B, C, T, R, idx, val[i], np.diag(sigma[i] ** 2), S=S)
        inv = np.argsort(perm)  # new variable j is old variable inv[j]
        a = order
        out["T"].append(T[np.ix_(inv, inv)])
        out["R"].append(R[inv])
        out["g_yy"].append(sol["g_yy"][inv][:, a][:, :, a])
        out["g_yu"].append(sol["g_yu"][inv][:, a])
        out["g_uu"].append(sol["g_uu"][inv])
        out["g_ss"].append(sol["g_ss"][inv])
    res = {key: np.ascontiguousarray(np.stack(v)) for key, v in out.items()}
    res["S"] = np.sort(perm[:s]).astype(np.int32)
    res["sigma"] = sigma
    for v in res.values():
        v.setflags(write=False)
    return res


def draw(c, i):
    """(T, R, sol) of draw ``i`` of a ``case``."""
    return c["T"][i], c["R"][i], dict(g_yy=c["g_yy"][i], g_yu=c["g_yu"][i], g_uu=c["g_uu"][i], g_ss=c["g_ss"][i], S=c["S"])


def solution(c):
    """The seven solution arguments of the public functions, as a dict."""
    return {key: c[key] for key in ("T", "R", "g_yy", "g_yu", "g_uu", "g_ss", "S")}
