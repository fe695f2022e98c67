"""Inputs and references of the anticipated-shock tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): built once,
read-only, shared by tests/test_anticipated_reference.py (CPU) and tests/test_gpu_anticipated.py.

On the SW-shaped generator as it stands the shocks enter the exogenous rows only and C loads on the lead columns only, so G R is
zero to rounding and anticipation does nothing.  The SW-shaped cases here therefore take (B, C, T_star) of the generator with a
DENSE impact matrix D = randn(n, k) / sqrt(n) and R = -M^-1 D (T does not depend on D); ``relevance`` measures, from the
reference alone, that anticipation matters in every case."""
import functools

import numpy as np

import oracle
from geconpy_amd import workloads as wl

from tests import anticipated_reference as ref
from tests.shock_decomposition_cases import SW

NB = 3
COND_BAR = 1e5    # cond_2(M) of every accuracy case, by the reference alone
RELEVANCE = 0.05  # max_{j >= 1} |G^j R| / |R| (Frobenius) of every accuracy case, by the reference alone


@functools.lru_cache(maxsize=None)
def model(name):
    """dict(B, C, T (NB, n, n), D, R (NB, n, k)), every draw distinct: "rbc" (n = 8, k = 1), "full_nk" (24, 4) with the model's own
    D, and the SW-shaped sizes with a dense D."""
    if name in ("rbc", "full_nk"):
        b, _ = (wl.rbc_batch if name == "rbc" else wl.full_nk_batch)(NB)
        T = np.empty_like(b["A"])
        for i in range(NB):
            T[i], ok, _ = oracle.cycle_reduction.cycle_reduction_core(b["A"][i], b["B"][i], b["C"][i], 1000, 1e-12)
            assert ok
        D = np.array(b["D"])
    else:
        b = wl.sw_shaped_batch(NB, **SW[name])
        T = np.array(b["T_star"])
        n, k = T.shape[1], b["D"].shape[2]
        D = np.random.default_rng([53, *name.encode()]).standard_normal((NB, n, k)) / np.sqrt(n)
    B, C = np.array(b["B"]), np.array(b["C"])
    R = np.stack([np.linalg.solve(B[i] + C[i] @ T[i], -D[i]) for i in range(NB)])
    out = dict(B=B, C=C, T=T, D=D, R=R)
    for key, a in out.items():
        out[key] = np.ascontiguousarray(a, dtype=np.float64)
        out[key].setflags(write=False)
    return out


# model, mode, n_lead (news), n_steps, n_shock, n_paths, how eps varies ("shared": one set of paths for all draws, "draw"), how
# x0 varies (None: NULL, "shared": (n,), "paths": (n_paths, n), "draw": (NB, 1, n), "path": (NB, n_paths, n)), Z ("sel" / "dense" /
# None: p = 0), p, d given
CASES = {
    # n = 8, k = 1: one path, 40 steps, no observation equation
    "rbc_pf": dict(model="rbc", mode="perfect_foresight", n_steps=40, n_shock=40, n_paths=1, eps="shared", x0=None),
    # shocks BEYOND the horizon: one step, four shock steps
    "rbc_beyond": dict(model="rbc", mode="perfect_foresight", n_steps=1, n_shock=4, n_paths=2, eps="draw", x0="path", Z="sel", p=2, d=True),
    # n = 24, rho(G) = 0.99: shocks end before the horizon, 17 paths (two groups), dense Z
    "nk_pf": dict(model="full_nk", mode="perfect_foresight", n_steps=40, n_shock=12, n_paths=17, eps="draw", x0="draw", Z="dense", p=3, d=True),
    "nk_news5": dict(model="full_nk", mode="news", n_lead=5, n_steps=40, n_shock=40, n_paths=16, eps="draw", x0="path", Z="sel", p=4),
    "sw16_news1": dict(model="sw16", mode="news", n_lead=1, n_steps=8, n_shock=5, n_paths=3, eps="shared", x0="shared"),
    "sw17_pf": dict(model="sw17", mode="perfect_foresight", n_steps=2, n_shock=2, n_paths=17, eps="draw", x0=None, Z="dense", p=5, d=True),
    "sw17_news0": dict(model="sw17", mode="news", n_lead=0, n_steps=6, n_shock=6, n_paths=2, eps="draw", x0="paths"),
    # the shape of the timing tool
    "sw40_pf": dict(model="sw40", mode="perfect_foresight", n_steps=40, n_shock=40, n_paths=16, eps="draw", x0="path", Z="sel", p=7),
    "sw40_news5": dict(model="sw40", mode="news", n_lead=5, n_steps=10, n_shock=7, n_paths=17, eps="draw", x0="draw", Z="sel", p=7, d=True),
    "sw49_above": dict(model="sw49", mode="perfect_foresight", n_steps=6, n_shock=9, n_paths=2, eps="shared", x0="draw", Z="dense", p=16),
    # n = 64, k = 8
    "sw64_pf": dict(model="sw64", mode="perfect_foresight", n_steps=12, n_shock=12, n_paths=17, eps="draw", x0="path", Z="sel", p=16, d=True),
    "sw64_news1": dict(model="sw64", mode="news", n_lead=1, n_steps=2, n_shock=1, n_paths=1, eps="draw", x0=None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of ``CASES[name]`` as ``batched.anticipated_paths_batched`` takes them (B, C, T, R, eps, x0, Z, d, mode, n_steps),
    plus D and the full arrays ``E (NB, n_paths, n_shock[, n_lead + 1], k)`` and ``X0 (NB, n_paths, n)``."""
    s = CASES[name]
    rng = np.random.default_rng([31, *name.encode()])
    mdl = model(s["model"])
    n, k = mdl["R"].shape[1:]
    n_paths, n_shock, news = s["n_paths"], s["n_shock"], s["mode"] == "news"
    tail = (n_shock, s.get("n_lead", 0) + 1, k) if news else (n_shock, k)
    lead = (1,) if s["eps"] == "shared" else (NB,)
    E = np.broadcast_to(0.01 * rng.standard_normal(lead + (n_paths,) + tail), (NB, n_paths) + tail).copy()
    eps = E[0] if s["eps"] == "shared" else E
    kind = s["x0"]
    lead = {None: (1, 1), "shared": (1, 1), "paths": (1, n_paths), "draw": (NB, 1), "path": (NB, n_paths)}[kind]
    X0 = np.broadcast_to(0.05 * rng.standard_normal(lead + (n,)), (NB, n_paths, n)).copy()
    if kind is None:
        X0[:] = 0.0
    x0 = {None: None, "shared": X0[0, 0], "paths": X0[0], "draw": X0[:, :1], "path": X0}[kind]
    p = s.get("p", 0)
    Z = d = None
    if s.get("Z") == "sel":
        Z = np.eye(p, n)
    elif s.get("Z") == "dense":
        Z = rng.standard_normal((p, n)) * (rng.random((p, n)) < 0.3)
        Z[np.arange(p), np.arange(p)] = 1.0
    if s.get("d"):
        d = rng.normal(0, 0.01, p)
    c = dict(mdl, eps=np.ascontiguousarray(eps), x0=None if x0 is None else np.ascontiguousarray(x0), Z=Z, d=d, mode=s["mode"],
             n_steps=s["n_steps"], n_paths=n_paths, n_shock=n_shock, n_lead=s.get("n_lead", 0), E=E, X0=X0, n=n, k=k, p=p)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def kwargs(c):
    """The keyword arguments of the public entries for case dict ``c``."""
    return dict(n_steps=c["n_steps"], mode=c["mode"], x0=c["x0"], Z=c["Z"], d=c["d"])


def outputs(c):
    return ("x", "w", "G") + (("observed",) if c["p"] else ())


def relevance(G, R, powers=64):
    """max_{j = 1 .. powers} |G^j R| / |R| (Frobenius): how much a shock known j periods ahead moves the path today."""
    best, GR = 0.0, R
    for _ in range(powers):
        GR = G @ GR
        best = max(best, np.linalg.norm(GR))
    return best / np.linalg.norm(R)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(x, w (NB, n_paths, n_steps, n), observed (.., p) or None, G (NB, n, n), cond (NB,): cond_2(M), relevance (NB,)) of the
    numpy reference; computed once, shared, never modified."""
    c = case(name)
    n_paths, n_steps, n, p = c["n_paths"], c["n_steps"], c["n"], c["p"]
    out = dict(x=np.empty((NB, n_paths, n_steps, n)), w=np.empty((NB, n_paths, n_steps, n)),
               observed=np.empty((NB, n_paths, n_steps, p)) if p else None, G=np.empty((NB, n, n)), cond=np.empty(NB),
               relevance=np.empty(NB))
    for b in range(NB):
        for s in range(n_paths):
            r = ref.anticipated_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], c["E"][b, s], n_steps, c["mode"], c["X0"][b, s],
                                      c["Z"], c["d"])
            out["x"][b, s], out["w"][b, s] = r["x"], r["w"]
            if p:
                out["observed"][b, s] = r["observed"]
        out["G"][b] = r["G"]
        out["cond"][b] = np.linalg.cond(r["M"])
        out["relevance"][b] = relevance(r["G"], c["R"][b])
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out
