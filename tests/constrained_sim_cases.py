"""Inputs and references of the tests of the stochastic simulation at an occasionally binding bound (TEST INFRASTRUCTURE ONLY; a
helper, not a test module): built once, read-only, shared by tests/test_constrained_sim_reference.py (CPU) and
tests/test_gpu_constrained_sim.py.  The models are those of tests/anticipated_cases.py, the construction that of
tests/constrained_cases.py.

Shocks are ``0.01 N(0, 1)``, surprises in every one of the ``n_shock`` periods.  The constraint row of a case is +- the unit vector
of the ``rank``-th most-moved variable of the constrained shock column, signed so that ``diag(Mz) = c'R[:, s] > 0``.  The bound is
``frac`` times the minimum of the UNCONSTRAINED simulated ``c'x`` (``x[t] = T x[t-1] + R eps[t]``) of the draw (of all draws for a
shared bound): 0.5 binds where the path dips, 2 never binds."""
import functools

import numpy as np

from tests import anticipated_cases as ac
from tests import anticipated_reference as aref
from tests import constrained_sim_reference as ref

NB = ac.NB
COND_BAR = ac.COND_BAR
COND_S_BAR = 1e5   # cond_2(Mz[S, S]) at every period's final S
MARGIN_BAR = 1e-6  # the smallest |decision quantity| of every period, in units of that period's max|q| (tests/constrained_cases.py)

# model; H; n_steps; n_shock; n_paths; shock ("first" / "last" column, or its index); rank; frac; shared (c and bound shared by the
# draws, else per draw); x0 (None / "draw" / "path"); Z ("sel" / "dense" / None), p, d; short: the HORIZON_SHORT bit is expected;
# fails: a failure case, not an accuracy case; t0: shocks at t = 0 only (time consistency)
CASES = {
    # n = 8, k = 1 (s = 0 = k - 1): the bound never binds
    "rbc_none": dict(model="rbc", H=2, n_steps=6, n_shock=4, n_paths=1, shock="first", rank=0, frac=2.0, shared=True, x0=None),
    "rbc_h8": dict(model="rbc", H=8, n_steps=24, n_shock=24, n_paths=5, shock="first", rank=0, frac=0.5, shared=True, x0="draw",
                   Z="sel", p=2, d=True),
    # H = 1: the plan is the realised shadow shock alone, and its last period binds whenever it binds
    "sw17_h1": dict(model="sw17", H=1, n_steps=6, n_shock=6, n_paths=17, shock="last", rank=0, frac=0.5, shared=False, x0="path",
                    short=True),
    "sw17_h17": dict(model="sw17", H=17, n_steps=20, n_shock=20, n_paths=5, shock="first", rank=1, frac=0.3, shared=False, x0=None,
                     Z="dense", p=5, short=True),
    # the last period of the plan binds
    "sw17_short": dict(model="sw17", H=17, n_steps=20, n_shock=12, n_paths=1, shock="first", rank=0, frac=0.5, shared=False, x0=None,
                       short=True, seed=1),
    "nk_h17": dict(model="full_nk", H=17, n_steps=40, n_shock=40, n_paths=5, shock=2, rank=3, frac=0.2, shared=False, x0=None,
                   Z="dense", p=3, d=True),
    # the shape of the timing tool but for 5 paths: up to 16 regime iterations in a period
    "sw40_h32": dict(model="sw40", H=32, n_steps=40, n_shock=40, n_paths=5, shock="first", rank=1, frac=0.3, shared=False, x0=None,
                     Z="sel", p=7, short=True, seed=4),
    # H > n_steps
    "sw40_h33": dict(model="sw40", H=33, n_steps=12, n_shock=12, n_paths=5, shock="last", rank=0, frac=0.5, shared=False, x0="draw"),
    # n = 64, k = 8, H = 64 > n_steps
    "sw64_h64": dict(model="sw64", H=64, n_steps=16, n_shock=16, n_paths=5, shock="last", rank=3, frac=0.3, shared=False, x0="path",
                     Z="sel", p=16, d=True, seed=1),
    # shocks at t = 0 only, n_steps = 2 H: the perfect-foresight path of the ABI 18 entry (time consistency)
    "rbc_t0": dict(model="rbc", H=8, n_steps=16, n_shock=1, n_paths=5, shock="first", rank=0, frac=0.5, shared=False, x0=None, t0=True,
                   short=True),
    "sw17_t0": dict(model="sw17", H=17, n_steps=34, n_shock=1, n_paths=5, shock="first", rank=1, frac=0.3, shared=False, x0=None,
                    t0=True, short=True),
    "sw40_t0": dict(model="sw40", H=32, n_steps=64, n_shock=1, n_paths=5, shock="first", rank=1, frac=0.3, shared=False, x0=None,
                    t0=True, seed=6),
    "sw64_t0": dict(model="sw64", H=64, n_steps=128, n_shock=1, n_paths=1, shock="last", rank=1, frac=0.3, shared=False, x0=None,
                    t0=True),
    # Mz is no P-matrix: some period ends without a regime
    "nk_fails": dict(model="full_nk", H=17, n_steps=40, n_shock=40, n_paths=5, shock="first", rank=0, frac=0.3, shared=False, x0=None,
                     fails=True),
}
ACCURACY = sorted(n for n, s in CASES.items() if not s.get("fails"))
TIME_CONSISTENCY = sorted(n for n, s in CASES.items() if s.get("t0"))


def _shock(s, k):
    return {"first": 0, "last": k - 1}.get(s["shock"], s["shock"])


def simulate_unconstrained(T, R, eps, n_steps, x0):
    """x (n_steps, n): x[t] = T x[t-1] + R eps[t], zero shocks after the rows of eps."""
    w = np.zeros((n_steps, T.shape[0]))
    w[:eps.shape[0]] = eps @ R.T
    return aref.propagate(T, w, x0)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of ``CASES[name]`` as ``batched.constrained_simulate_batched`` takes them (B, C, T, R, eps, c, bound, shock, horizon,
    n_steps, x0, Z, d), plus D and the full arrays ``E (NB, n_paths, n_shock, k)``, ``X0 (NB, n_paths, n)``, ``Cr (NB, n)`` and
    ``Bd (NB,)``."""
    s = CASES[name]
    rng = np.random.default_rng([59, s.get("seed", 0), *name.encode()])
    mdl = ac.model(s["model"])
    n, k = mdl["R"].shape[1:]
    sh, H, n_paths, n_shock, n_steps = _shock(s, k), s["H"], s["n_paths"], s["n_shock"], s["n_steps"]
    Rs = mdl["R"][0 if s["shared"] else slice(None), :, sh].reshape(-1, n)
    var = np.broadcast_to(np.argsort(-np.abs(Rs), axis=1)[:, s["rank"]], (NB,))
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
    cx = np.empty((NB, n_paths, n_steps))
    for b in range(NB):
        for j in range(n_paths):
            cx[b, j] = simulate_unconstrained(mdl["T"][b], mdl["R"][b], E[b, j], n_steps, X0[b, j]) @ Cr[b]
    Bd = np.broadcast_to(s["frac"] * cx.min(axis=None if s["shared"] else (1, 2)), (NB,)).copy()
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
             X0=X0, Cr=Cr, Bd=Bd, n=n, k=k, p=p, short=bool(s.get("short")))
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
    return ("x", "gap", "shadow", "plan", "duration", "iters", "Mz", "path_status", "fail_step") + (("observed",) if c["p"] else ())


@functools.lru_cache(maxsize=None)
def reference(name, max_iter=0):
    """dict(x (NB, n_paths, n_steps, n), observed (.., p) or None, gap, shadow (NB, n_paths, n_steps), plan (.., H), duration, iters
    (NB, n_paths, n_steps) int32, path_status, fail_step (NB, n_paths) int32, Mz (NB, H, H), q (NB, n_paths, n_steps, H), S (same)
    bool, qmax (NB, n_paths, n_steps), margin (NB, n_paths), cond (NB,): cond_2(M), cond_S (NB, n_paths): the largest
    cond_2(Mz[S, S]) over the periods' final S) of the numpy reference; computed once, shared, never modified."""
    c = case(name)
    n_paths, n_steps, n, p, H = c["n_paths"], c["n_steps"], c["n"], c["p"], c["horizon"]
    f = lambda *sh: np.empty((NB, n_paths) + sh)  # noqa: E731
    g = lambda *sh: np.empty((NB, n_paths) + sh, np.int32)  # noqa: E731
    out = dict(x=f(n_steps, n), observed=f(n_steps, p) if p else None, gap=f(n_steps), shadow=f(n_steps), plan=f(n_steps, H),
               duration=g(n_steps), iters=g(n_steps), path_status=g(), fail_step=g(), q=f(n_steps, H),
               S=np.empty((NB, n_paths, n_steps, H), bool), qmax=f(n_steps), margin=f(), cond_S=f(), Mz=np.empty((NB, H, H)),
               cond=np.empty(NB))
    for b in range(NB):
        for j in range(n_paths):
            r = ref.constrained_simulate(c["B"][b], c["C"][b], c["T"][b], c["R"][b], c["E"][b, j], c["Cr"][b], c["Bd"][b], c["shock"], H,
                                         n_steps, c["X0"][b, j], c["Z"], c["d"], max_iter=max_iter)
            for key in ("x", "gap", "shadow", "plan", "duration", "iters", "q", "S", "qmax", "margin", "fail_step"):
                out[key][b, j] = r[key]
            if p:
                out["observed"][b, j] = r["observed"]
            out["path_status"][b, j] = r["status"]
            sets = {tuple(S) for S in r["S"] if S.any()}
            out["cond_S"][b, j] = max((np.linalg.cond(r["Mz"][np.ix_(S, S)]) for S in map(np.array, sets)), default=1.0)
        out["Mz"][b] = r["Mz"]
        out["cond"][b] = np.linalg.cond(r["M"])
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out
