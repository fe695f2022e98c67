"""Inputs and references of the conditional-forecast tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): built once,
read-only, shared by tests/test_conditional_forecast_reference.py (CPU) and tests/test_gpu_conditional_forecast.py."""
import functools

import numpy as np

from tests import conditional_forecast_reference as ref
from tests.shock_decomposition_cases import model

NB = 3
COND_BAR = 1e5  # every case used for accuracy: cond_2(G) of the REFERENCE at most this (rounding of the solve then stays near 1e-11)


def _grid(periods, series):
    return [(t, j) for t in periods for j in series]


# model, p, Z ("sel" = eye(p, m) / "dense"), q (the four layouts), d given, free shocks (None = all), the (t, j) pairs, n_steps,
# n_paths, and how x0 / eps / the values vary: "shared", "draw" (per draw), "path" (per draw and path); eps None = NULL;
# n_shock = the steps of eps
CASES = {
    # m = 8, k = 1, p = 1: square (one series per period, one shock), one path
    "rbc_square": dict(model="rbc", p=1, conds=_grid(range(4), [0]), n_steps=6, n_paths=1, q="diag", x0="draw", vals="draw"),
    # m = 16: per-path everything, d given, diagonal Q per draw
    "sw16_paths": dict(model="sw16", p=3, conds=_grid(range(4), [0, 2]), n_steps=8, n_paths=16, q="diag_batched", d=True, eps="draw",
                       n_shock=8, x0="path", vals="path"),
    "sw16_p1": dict(model="sw16", p=1, conds=_grid([1, 3], [0]), n_steps=5, n_paths=2, q="diag", x0="shared", vals="shared"),
    # m = 17: dense Z, full Q, a gap in the conditioned periods, 17 paths (two groups), shared eps that ends before n_steps
    "sw17_gap": dict(model="sw17", p=4, Z="dense", conds=_grid([0, 1, 2, 5, 6], [1, 3]), n_steps=9, n_paths=17, q="full", eps="shared",
                     n_shock=5, x0="draw", vals="draw"),
    # a proper subset of free shocks with a full Q per draw: the block Q_FF
    "sw17_subset": dict(model="sw17", p=4, conds=_grid(range(5), [0]), free=[0, 2], n_steps=7, n_paths=3, q="full_batched", d=True,
                        eps="draw", n_shock=7, x0="path", vals="draw"),
    # conditions at t = 0 only
    "sw17_t0": dict(model="sw17", p=2, conds=[(0, 0), (0, 1)], n_steps=5, n_paths=2, q="diag", x0="shared", vals="shared"),
    # the square case of the issue: observables {0, 1}, shocks {0, 1}
    "sw17_square": dict(model="sw17", p=2, conds=_grid(range(6), [0, 1]), free=[0, 1], n_steps=8, n_paths=2, q="full", eps="draw",
                        n_shock=8, x0="draw", vals="path"),
    # m = 40: 36 conditions up to the LAST step
    "sw40_last": dict(model="sw40", p=7, conds=_grid(range(12), [0, 2, 4]), n_steps=12, n_paths=16, q="diag_batched", d=True,
                      eps="draw", n_shock=12, x0="path", vals="path"),
    # n_cond = 64, square
    "sw40_square64": dict(model="sw40", p=7, conds=_grid(range(32), [0, 1]), free=[0, 1], n_steps=32, n_paths=2, q="diag", x0="draw",
                          vals="draw"),
    # 40 steps, the shape of the timing tool
    "sw40_40steps": dict(model="sw40", p=7, conds=_grid(range(12), [0, 2, 4]), n_steps=40, n_paths=16, q="diag", eps="draw", n_shock=40,
                         x0="path", vals="path"),
    "sw49_dense": dict(model="sw49", p=5, Z="dense", conds=_grid(range(3), [0, 1, 4]), n_steps=6, n_paths=17, q="full_batched", d=True,
                       eps="draw", n_shock=3, x0="draw", vals="path"),
    "sw64_p16": dict(model="sw64", p=16, conds=_grid(range(4), [0, 1, 2]), n_steps=6, n_paths=1, q="diag_batched", d=True, x0="draw",
                     vals="draw"),
    "sw96": dict(model="sw96", p=3, conds=_grid(range(6), [0, 2]), n_steps=8, n_paths=3, q="full", d=True, eps="draw", n_shock=8,
                 x0="path", vals="path"),
}


def _full_q(sigma, rng):
    L = np.diag(sigma) + 0.25 * np.tril(rng.standard_normal((len(sigma),) * 2), -1) * sigma.mean()
    return L @ L.T


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of ``CASES[name]`` as ``batched.conditional_forecast_batched`` takes them, plus ``cond_t`` / ``cond_j`` and the full
    arrays ``X0 (nb, n_paths, m)``, ``E (nb, n_paths, n_shock, k)`` or None, ``V (nb, n_paths, n_cond)``, ``Qf (nb, k, k)``."""
    s = CASES[name]
    rng = np.random.default_rng([29, *name.encode()])
    T, R = model(s["model"], NB)
    m, k = R.shape[1:]
    p, n_steps, n_paths = s["p"], s["n_steps"], s["n_paths"]
    if s.get("Z", "sel") == "sel":
        Z = np.eye(p, m)
    else:
        Z = rng.standard_normal((p, m)) * (rng.random((p, m)) < 0.3)
        Z[np.arange(p), np.arange(p)] = 1.0
    d = rng.normal(0, 0.01, p) if s.get("d") else None
    sigma = rng.uniform(0.005, 0.02, (NB, k))
    q = {"diag": lambda: sigma[0] ** 2, "diag_batched": lambda: sigma ** 2, "full": lambda: _full_q(sigma[0], rng),
         "full_batched": lambda: np.stack([_full_q(sigma[i], rng) for i in range(NB)])}[s["q"]]()
    Qf = np.stack([(np.diag(qi) if qi.ndim == 1 else qi) for qi in (q if s["q"].endswith("batched") else [q] * NB)])

    def vary(kind, tail, scale):
        lead = {"shared": (1, 1), "draw": (NB, 1), "path": (NB, n_paths)}[kind]
        return np.broadcast_to(scale * rng.standard_normal(lead + tail), (NB, n_paths) + tail).copy()

    X0 = vary(s["x0"], (m,), 0.05)
    E = None
    if s.get("eps"):
        E = vary("path" if s["eps"] == "draw" else "shared", (s["n_shock"], k), 1.0)
        E *= sigma[:, None, None, :] if s["eps"] == "draw" else sigma[0]
    ct, cj = (np.array(v, dtype=np.int32) for v in zip(*s["conds"]))
    V = vary(s["vals"], (len(ct),), 0.02)
    x0 = {"shared": X0[0, 0], "draw": X0[:, 0], "path": X0}[s["x0"]]
    eps = None if E is None else (E if s["eps"] == "draw" else E[0])
    vals = {"shared": V[0, 0], "draw": V[:, 0], "path": V}[s["vals"]]
    shape = {"shared": (), "draw": (NB,), "path": (NB, n_paths)}[s["vals"]]
    conditions = np.full(shape + (int(ct.max()) + 1, p), np.nan)
    conditions[..., ct, cj] = vals
    c = dict(T=T, R=R, Q=q, q_mode=s["q"], Z=Z, d=d, x0=np.ascontiguousarray(x0), eps=None if eps is None else np.ascontiguousarray(eps),
             conditions=conditions, free=s.get("free"), n_steps=n_steps, n_paths=n_paths, cond_t=ct, cond_j=cj, X0=X0, E=E, V=V, Qf=Qf,
             m=m, k=k, p=p)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def kwargs(c):
    """The keyword arguments of the public entries for case dict ``c``."""
    return dict(Z=c["Z"], d=c["d"], eps=c["eps"], n_paths=c["n_paths"], free_shocks=c["free"], q_mode=c["q_mode"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(x (nb, n_paths, n_steps, m), shocks, observed, cond (nb,): cond_2(G) per draw) of the numpy reference; computed once,
    shared, never modified."""
    c = case(name)
    nb, n_paths, n_steps = NB, c["n_paths"], c["n_steps"]
    out = dict(x=np.empty((nb, n_paths, n_steps, c["m"])), shocks=np.empty((nb, n_paths, n_steps, c["k"])),
               observed=np.empty((nb, n_paths, n_steps, c["p"])), cond=np.empty(nb))
    F = np.arange(c["k"]) if c["free"] is None else np.asarray(sorted(c["free"]))
    for b in range(nb):
        WQ = ref.system(c["T"][b], c["R"][b], c["Qf"][b], c["Z"], c["cond_t"], c["cond_j"], F)
        for s in range(n_paths):
            r = ref.conditional_forecast(c["T"][b], c["R"][b], c["Qf"][b], c["Z"], c["d"], c["X0"][b, s], c["cond_t"], c["cond_j"],
                                         c["V"][b, s], n_steps, eps=None if c["E"] is None else c["E"][b, s], free=F, WQ=WQ)
            for key in ("x", "shocks", "observed"):
                out[key][b, s] = r[key]
        out["cond"][b] = np.linalg.cond(r["G"])
    for a in out.values():
        a.setflags(write=False)
    return out
