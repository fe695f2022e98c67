"""Inputs and references of the occasionally-binding-bound tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): built
once, read-only, shared by tests/test_constrained_reference.py (CPU) and tests/test_gpu_constrained.py.  The models are those of
tests/anticipated_cases.py.

The constraint row of a case is +- the unit vector of the variable that the constrained shock column moves most on impact (the
``rank``-th most, for cases that say so), signed so that ``diag(Mz) = c'R[:, s] > 0``.  The bound follows a rule on the unconstrained
paths ``c'xu`` of the draw (of all draws for a shared bound): ``("frac", f)``: ``f`` times their minimum over paths and periods --
0.5 binds where the path dips, 2 never binds; ``("above", f)``: their maximum over ``t < H`` plus ``f`` times their range, so that
every period binds."""
import functools

import numpy as np

from tests import anticipated_cases as ac
from tests import anticipated_reference as aref
from tests import constrained_reference as ref

NB = ac.NB
COND_BAR = ac.COND_BAR
MARGIN_BAR = 1e-6  # the smallest |decision quantity| of every path, and its gap beyond the horizon, in units of max|q|


def unit_impact_model(name, s, i):
    """``ac.model(name)`` with ``D[:, s] = e_i`` and R recomputed."""
    mdl = ac.model(name)
    D = mdl["D"].copy()
    D[:, :, s] = 0.0
    D[:, i, s] = 1.0
    R = np.stack([np.linalg.solve(mdl["B"][b] + mdl["C"][b] @ mdl["T"][b], -D[b]) for b in range(NB)])
    return dict(mdl, D=D, R=R)


# model; H; n_steps; n_shock; n_paths; shock ("first" / "last" column); rank (0: the most-moved variable); shared (c and bound
# shared by the draws, else per draw); bound rule; x0 (None / "path" / "draw"); Z ("sel" / "dense" / None), p, d;
# unit: D[:, s] = e_i for the constrained variable i
CASES = {
    # n = 8, k = 1 (s = 0 = k - 1): nothing binds; n_shock_steps below H
    "rbc_none": dict(model="rbc", H=2, n_steps=5, n_shock=1, n_paths=1, shock="first", shared=True, bound=("frac", 2.0), x0=None),
    # every period binds, H = n_steps = n_shock_steps
    "rbc_all": dict(model="rbc", H=2, n_steps=2, n_shock=2, n_paths=5, shock="last", shared=False, bound=("above", 0.5), x0="path",
                    Z="sel", p=2, d=True),
    # H = 1 and shocks beyond n_steps: binding at t = 0 on the paths below the bound
    "sw17_h1": dict(model="sw17", H=1, n_steps=1, n_shock=3, n_paths=17, shock="last", shared=False, bound=("frac", 0.5), x0="path"),
    # n = 24, rho(G) = 0.99: several regime iterations
    "nk_iters": dict(model="full_nk", H=17, n_steps=40, n_shock=12, n_paths=5, shock=2, rank=3, shared=False, bound=("frac", 0.5),
                     x0=None, Z="dense", p=3, d=True),
    # the shape of the timing tool but for 17 paths; shocks for the first 8 periods
    "sw40_h32": dict(model="sw40", H=32, n_steps=40, n_shock=8, n_paths=17, shock="first", shared=False, bound=("frac", 0.5),
                     x0=None, Z="sel", p=7),
    "sw40_h33": dict(model="sw40", H=33, n_steps=33, n_shock=33, n_paths=5, shock="last", shared=False, bound=("frac", 0.5),
                     x0="draw"),
    "sw17_h17": dict(model="sw17", H=17, n_steps=17, n_shock=20, n_paths=1, shock="first", shared=True, bound=("frac", 0.5),
                     x0=None, Z="dense", p=5, unit=True),
    # n = 64, k = 8
    "sw64_h64": dict(model="sw64", H=64, n_steps=64, n_shock=64, n_paths=5, shock="last", shared=False, bound=("frac", 0.5),
                     x0="path", Z="sel", p=16, d=True, unit=True),
    # a unit-vector impact column on the two remaining models of the stacked-time test
    "rbc_unit": dict(model="rbc", H=8, n_steps=12, n_shock=4, n_paths=1, shock="first", shared=False, bound=("frac", 0.5), x0="draw",
                     unit=True),
    "sw40_unit": dict(model="sw40", H=33, n_steps=40, n_shock=6, n_paths=5, shock="first", shared=False, bound=("frac", 0.5),
                      x0=None, unit=True),
    # the bound is violated after the horizon: reported, not repaired
    "rbc_beyond": dict(model="rbc", H=2, n_steps=12, n_shock=6, n_paths=5, shock="first", shared=False, bound=("frac", 0.5),
                       x0=None, beyond=True),
}


def _shock(s, k):
    return {"first": 0, "last": k - 1}.get(s["shock"], s["shock"])


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of ``CASES[name]`` as ``batched.constrained_paths_batched`` takes them (B, C, T, R, eps, c, bound, shock, horizon,
    n_steps, x0, Z, d), plus D and the full arrays ``E (NB, n_paths, n_shock, k)``, ``X0 (NB, n_paths, n)``, ``Cr (NB, n)`` and
    ``Bd (NB,)``."""
    s = CASES[name]
    rng = np.random.default_rng([37, *name.encode()])
    mdl = ac.model(s["model"])
    n, k = mdl["R"].shape[1:]
    sh, H, n_paths, n_shock, n_steps = _shock(s, k), s["H"], s["n_paths"], s["n_shock"], s["n_steps"]
    # the constrained variable, by the model as it stands
    Rs = mdl["R"][0 if s["shared"] or s.get("unit") else slice(None), :, sh].reshape(-1, n)
    var = np.broadcast_to(np.argsort(-np.abs(Rs), axis=1)[:, s.get("rank", 0)], (NB,))
    if s.get("unit"):
        mdl = unit_impact_model(s["model"], sh, int(var[0]))
    Cr = np.zeros((NB, n))
    Cr[np.arange(NB), var] = np.sign(mdl["R"][np.arange(NB), var, sh])
    if s["shared"]:
        assert (Cr == Cr[0]).all()
    E = 0.01 * rng.standard_normal((NB, n_paths, n_shock, k))
    lead = {None: (1, 1), "draw": (NB, 1), "path": (NB, n_paths)}[s["x0"]]
    X0 = np.broadcast_to(0.05 * rng.standard_normal(lead + (n,)), (NB, n_paths, n)).copy()
    if s["x0"] is None:
        X0[:] = 0.0
    x0 = {None: None, "draw": X0[:, :1], "path": X0}[s["x0"]]
    # the bound, from the unconstrained paths
    cx = np.empty((NB, n_paths, n_steps))
    for b in range(NB):
        G, _ = aref.gain(mdl["B"][b], mdl["C"][b], mdl["T"][b])
        for j in range(n_paths):
            w = aref.anticipation(G, mdl["R"][b], E[b, j], n_steps, "perfect_foresight")
            cx[b, j] = aref.propagate(mdl["T"][b], w, X0[b, j]) @ Cr[b]
    rule, f = s["bound"]
    axes = None if s["shared"] else (1, 2)
    if rule == "frac":
        Bd = f * cx.min(axis=axes)
    else:
        Bd = cx[:, :, :H].max(axis=axes) + f * (cx[:, :, :H].max(axis=axes) - cx[:, :, :H].min(axis=axes))
    Bd = np.broadcast_to(Bd, (NB,)).copy()
    p = s.get("p", 0)
    Z = d = None
    if s.get("Z") == "sel":
        Z = np.eye(p, n)
    elif s.get("Z") == "dense":
        Z = rng.standard_normal((p, n)) * (rng.random((p, n)) < 0.3)
        Z[np.arange(p), np.arange(p)] = 1.0
    if s.get("d"):
        d = rng.normal(0, 0.01, p)
    c = dict(mdl, eps=E, x0=None if x0 is None else np.ascontiguousarray(x0), Z=Z, d=d, c=Cr[0].copy() if s["shared"] else Cr,
             bound=float(Bd[0]) if s["shared"] else Bd, shock=sh, horizon=H, n_steps=n_steps, n_paths=n_paths, n_shock=n_shock, E=E,
             X0=X0, Cr=Cr, Bd=Bd, n=n, k=k, p=p, beyond=bool(s.get("beyond")))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def kwargs(c):
    """The keyword arguments of the public entries for case dict ``c`` (after B, C, T, R, eps, c, bound, shock, horizon)."""
    return dict(n_steps=c["n_steps"], x0=c["x0"], Z=c["Z"], d=c["d"])


def args(c):
    return c["B"], c["C"], c["T"], c["R"], c["eps"], c["c"], c["bound"], c["shock"], c["horizon"]


def outputs(c):
    return ("x", "w", "nu", "gap", "Mz", "path_status", "iters") + (("observed",) if c["p"] else ())


@functools.lru_cache(maxsize=None)
def reference(name, max_iter=0):
    """dict(x, w (NB, n_paths, n_steps, n), observed (.., p) or None, nu (NB, n_paths, H), gap (NB, n_paths, n_steps), Mz (NB, H, H),
    q, S (NB, n_paths, H), iters, path_status, margin (NB, n_paths), qmax (NB, n_paths): max|q|, cond (NB,): cond_2(M), cond_S
    (NB, n_paths): cond_2(Mz[S, S]) at the final S) of the numpy reference; computed once, shared, never modified."""
    c = case(name)
    n_paths, n_steps, n, p, H = c["n_paths"], c["n_steps"], c["n"], c["p"], c["horizon"]
    f = lambda *sh: np.empty((NB, n_paths) + sh)  # noqa: E731
    out = dict(x=f(n_steps, n), w=f(n_steps, n), observed=f(n_steps, p) if p else None, nu=f(H), gap=f(n_steps), q=f(H),
               S=np.empty((NB, n_paths, H), bool), iters=np.empty((NB, n_paths), np.int32), path_status=np.empty((NB, n_paths), np.int32),
               margin=f(), qmax=f(), cond_S=f(), Mz=np.empty((NB, H, H)), cond=np.empty(NB))
    for b in range(NB):
        for j in range(n_paths):
            r = ref.constrained_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], c["E"][b, j], c["Cr"][b], c["Bd"][b], c["shock"], H,
                                      n_steps, c["X0"][b, j], c["Z"], c["d"], max_iter=max_iter)
            for key in ("x", "w", "nu", "gap", "q", "S", "iters", "margin"):
                out[key][b, j] = r[key]
            if p:
                out["observed"][b, j] = r["observed"]
            out["path_status"][b, j] = r["status"]
            out["qmax"][b, j] = np.abs(r["q"]).max()
            S = r["S"]
            out["cond_S"][b, j] = np.linalg.cond(r["Mz"][np.ix_(S, S)]) if S.any() else 1.0
        out["Mz"][b] = r["Mz"]
        out["cond"][b] = np.linalg.cond(r["M"])
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def spells(S):
    """The number of separate runs of binding periods in S (H,) bool."""
    return int(S[0]) + int((S[1:] & ~S[:-1]).sum())
