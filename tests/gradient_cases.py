"""Inputs of the entry-by-entry gradient checks (TEST INFRASTRUCTURE ONLY; a helper, not a test module), as tests/smoother_cases.py
serves the smoother: tests/test_gradient_reference.py holds the autograd reference (tests/gradient_reference.py) to the oracle and
to itself on them, tests/test_gpu_gradient_entries.py the device to the reference -- the same arrays, built once, read-only.

A PROBLEM is the mathematical input: dict(A, B, C (nb, n, n), D (nb, n, k), q (k,) | (nb, k) or Q (k, k) | (nb, k, k), Z (p, n) |
(nb, p, n), y (T_len, p), d (p,), Hdiag (p,), conv: FilterConventions keywords or None, want_Z, draws: the draws that have a
reference).  A CASE is a problem plus the way it is sent through ``batched.solve_kalman_logp_grad_batched``: several cases (the
kernel routes, the two settings of kalman_steady_tol) share one problem and therefore one reference.  ``draw(pr, i)`` gives the
keyword arguments of ``gradient_reference.logp_and_gradient`` for one draw, ``reference(problem)`` the cached reference.

The shapes are the smallest that reach each kernel instance, taken from tests/test_gpu_gradient.py.  Unless its builder says
otherwise a problem has 2 draws, T_len = 40, one missing entry y[7, 1] and one all-missing row y[11].  The RBC model has a single
shock: "rbc" is also the n = 8, k = 1 case.

Every draw here has to pass the conditioning check of tests/test_gradient_reference.py (the reference gradient moves by at most
1e-8 of each block's scale under a 1e-11 relative perturbation of A, B, C, D); a draw that does not is replaced by another seed."""
import functools

import numpy as np

from geconpy_amd import workloads as wl

from tests import gradient_reference

T_LEN = 40
# (n, n_state, n_lead): the tiles of the reverse sweep (test_gradient_across_the_tiles_of_the_reverse_sweep,
# test_gradient_on_the_56_wide_tile); the last two hand over to the two-kernel adjoint path
TILES = ((20, 9, 5), (24, 14, 6), (40, 18, 12), (40, 22, 10), (44, 30, 8), (48, 34, 6), (52, 23, 15), (56, 25, 16), (40, 26, 10), (30, 20, 6))
EDGES = ("tlen1", "tlen2", "tlen3", "first_missing", "last_missing", "series_missing", "p1", "p8", "k1")
CONVENTIONS = {"conv_one_noP_maskd_plain": dict(ll_constant="one", jitter_on_F=True, jitter_on_P=False, mask_d=True, joseph=False),
               "conv_observed_maskd": dict(ll_constant="observed", jitter_on_F=True, jitter_on_P=True, mask_d=True, joseph=True),
               "conv_plain": dict(ll_constant="p", jitter_on_F=True, jitter_on_P=True, mask_d=False, joseph=False)}
SOLVE = dict(tol=1e-13, max_iter=200)
RBC_SEED = 4
# (rbc_tlen2, seed 4: q_bar of draw 1 cancels to 1e-4 of the other draw's, conditioning 1.4e-8.  rbc_p8: eight observed series and
#  one shock -- the two formulations of the reference agree to ~1e-12 only on most seeds, 7e-12 on seed 4; 8e-14 on seed 9)
RBC_SEEDS = {"rbc_tlen2": 7, "rbc_p8": 9}  # problem -> seed of rbc_prior_draws where a draw of RBC_SEED misses the floor or the conditioning check


def _tile_name(n, ns, nl):
    return f"sw{n}_{ns}_{nl}"


def _standard_missing(y):
    y = y.copy()
    if y.shape[0] > 11:
        y[7, min(1, y.shape[1] - 1)] = np.nan
        y[11, :] = np.nan
    return y


def _rbc(nb, p, seed=RBC_SEED):
    th = wl.rbc_prior_draws(nb, seed=seed)
    A, B, C, D = wl.rbc_linearized_jacobians(**th)
    names = ("Y", "C", "L")[:p] if p <= 3 else wl.RBC_VARIABLES
    Z = np.zeros((p, 8))
    for o, name in enumerate(names):
        Z[o, wl.RBC_VARIABLES.index(name)] = (1.0, 0.5, -2.0)[o] if p <= 3 else 1.0
    d = np.array([0.01, -0.02, 0.015, 0.0, 0.01, -0.01, 0.02, -0.015])[:p]
    h = np.array([1e-4, 2e-4, 1e-4, 1e-4, 2e-4, 1e-4, 1e-4, 2e-4])[:p]
    return dict(A=A, B=B, C=C, D=D, q=(th["sigma_A"] ** 2)[:, None], Z=Z, d=d, Hdiag=h)


def _sw(nb, rng, first_draw=0, observed=None, **shape):
    b = wl.sw_shaped_batch(nb, first_draw=first_draw, **shape)
    om = wl.sw_shaped_observation_model(observed=observed, **shape)
    p = om["Z"].shape[0]
    return dict(A=b["A"], B=b["B"], C=b["C"], D=b["D"], q=b["sigma"] ** 2, Z=om["Z"], d=rng.normal(0, 0.01, p), Hdiag=om["Hdiag"].copy(),
                y=om["y"])


def _edge(pr, edge, rng):
    """The sample edges on a model ``pr`` that carries a full panel ``y`` (T_LEN steps at least)."""
    y = pr["y"][:T_LEN]
    if edge.startswith("tlen"):
        y = y[:int(edge[4:])].copy()
        if y.shape[0] == 3:
            y[1, min(1, y.shape[1] - 1)] = np.nan
    else:
        y = _standard_missing(y)
        if edge == "first_missing":
            y[0, :] = np.nan
        elif edge == "last_missing":
            y[-1, :] = np.nan
        elif edge == "series_missing":
            y[:, 1] = np.nan
    pr["y"] = y
    return pr


def _finish(pr):
    pr.setdefault("conv", None)
    pr.setdefault("want_Z", False)
    pr.setdefault("draws", tuple(range(pr["A"].shape[0])))
    for a in pr.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def problem(name):
    rng = np.random.default_rng([23, *name.encode()])
    if name == "rbc" or name.startswith("rbc_"):
        edge = name[4:]
        if name in CONVENTIONS_RBC:
            # tests/test_gpu_conventions.py::rbc_case: 3 draws, 3 observed series, scattered missing entries and an all-missing step
            pr = _rbc(3, 3)
            y = rng.normal(0, 0.05, (T_LEN, 3))
            y[rng.random(y.shape) < 0.10] = np.nan
            y[3, :] = np.nan
            y[9, 2] = np.nan  # (mask_d: at least one missing entry whatever the scatter gave)
            return _finish(dict(pr, y=y, conv=CONVENTIONS[CONVENTIONS_RBC[name]]))
        p = {"p1": 1, "p8": 8}.get(edge, 2)
        pr = _rbc(2, p, RBC_SEEDS.get(name, RBC_SEED))
        pr["y"] = rng.normal(0, 0.05, (T_LEN, p))
        return _finish(_edge(pr, edge, rng) if edge else dict(pr, y=_standard_missing(pr["y"])))
    if name.startswith("sw40e_"):  # the sample edges on the 40-variable SW-shaped workload (n_state 18, n_lead 12, k = p = 7)
        edge = name[6:]
        shape = {"p1": dict(p=1), "p8": dict(p=8), "k1": dict(k=1)}.get(edge, {})
        return _finish(_edge(_sw(2, rng, T_len=T_LEN, **shape), edge, rng))
    if name in TILE_SHAPES or name == "sw40_jumps":
        n, ns, nl = (40, 18, 12) if name == "sw40_jumps" else TILE_SHAPES[name]
        observed = tuple(range(ns, ns + 7)) if name == "sw40_jumps" else None  # seven jump variables: u = 25 retained variables
        pr = _sw(2, rng, seed0=9100 + n + ns, observed=observed, n=n, n_state=ns, n_lead=nl, k=5, p=7, T_len=T_LEN)
        return _finish(dict(pr, y=_standard_missing(pr["y"])))
    if name == "sw40_failed_draw":  # 3 draws, the solver fails on draw 1
        pr = _sw(3, rng, T_len=T_LEN)
        A = pr["A"].copy()
        A[1, 0, 0] = np.nan
        return _finish(dict(pr, A=A, y=_standard_missing(pr["y"]), draws=(0, 2)))
    if name == "steady":  # test_gradient_with_steady_state_segments: two steady segments around a change of the mask
        pr = _sw(2, rng, T_len=130)
        y = pr["y"].copy()
        y[95, 1] = np.nan
        y[96, :] = np.nan
        return _finish(dict(pr, y=y))
    if name in ("q_shared", "Q_shared", "Q_batched"):
        pr = _sw(2, rng, first_draw=40, T_len=T_LEN)
        pr["y"] = _standard_missing(pr["y"])
        sigma = np.sqrt(pr["q"])
        if name == "q_shared":
            pr["q"] = pr["q"][0].copy()
        else:  # test_gradient_with_a_full_shock_covariance: Q = L L', L = diag(sigma) + 0.25 tril(N, -1) mean(sigma)
            k = sigma.shape[1]
            Ls = [np.diag(s) + 0.25 * np.tril(rng.standard_normal((k, k)), -1) * s.mean() for s in sigma]
            Q = np.stack([L @ L.T for L in Ls])
            del pr["q"]
            pr["Q"] = Q[0].copy() if name == "Q_shared" else Q
        return _finish(pr)
    if name in ("Z_shared", "Z_batched", "Z_selector"):
        pr = _sw(2, rng, first_draw=80, T_len=T_LEN)
        pr["y"] = _standard_missing(pr["y"])
        if name != "Z_selector":  # test_gradient_with_a_dense_design_matrix: a sixth of the entries of Z moved off the selector
            Zs = np.stack([pr["Z"] + 0.15 * rng.standard_normal(pr["Z"].shape) * (rng.random(pr["Z"].shape) < 0.15) for _ in range(2)])
            pr["Z"] = Zs[0].copy() if name == "Z_shared" else Zs
        return _finish(dict(pr, want_Z=True))
    raise KeyError(name)


TILE_SHAPES = {_tile_name(*s): s for s in TILES}
CONVENTIONS_RBC = {"rbc_" + k_: k_ for k_ in CONVENTIONS}


def _case(problem_name, **kw):
    return dict(problem=problem_name, kwargs=dict(SOLVE, **kw), refine=0)


def _cases():
    c = {"rbc": _case("rbc")}
    c.update({name: _case(name) for name in TILE_SHAPES})
    c["sw40_jumps"] = _case("sw40_jumps")
    for e in EDGES:
        if e != "k1":
            c["rbc_" + e] = _case("rbc_" + e)
        c["sw40e_" + e] = _case("sw40e_" + e)
    c["steady"] = _case("steady")
    c["steady_tol0"] = _case("steady", options={"kalman_steady_tol": 0.0})
    sw40 = _tile_name(40, 18, 12)
    for split in (0, 1, 2):
        c[f"route_split{split}"] = _case(sw40, options={"kalman_grad_split": split})
    c["route_refine"] = dict(_case(sw40), refine=1)  # dsge_debug_adjoint_refine(1): every draw takes the two-kernel adjoint path
    c["route_gensys"] = _case(sw40, solver="gensys", tol=1e-8)
    for name in ("q_shared", "Q_shared", "Q_batched"):
        c[name] = _case(name)
    c["Z_shared"] = _case("Z_shared", return_Z_bar=True)
    c["Z_batched"] = _case("Z_batched", return_Z_bar=True)
    c["Z_selector"] = _case("Z_selector", dense_z=True, return_Z_bar=True)
    c.update({name: _case(name) for name in CONVENTIONS_RBC})
    c["sw40_failed_draw"] = _case("sw40_failed_draw")
    return c


CASES = _cases()
PROBLEMS = tuple(dict.fromkeys(c["problem"] for c in CASES.values()))


def entry_point_arguments(name):
    """(positional A, B, C, D, q, Z, y; keyword arguments) of ``batched.solve_kalman_logp_grad_batched`` for a case.  The filter
    conventions of the problem are merged into ``options``."""
    from geconpy_amd import _lib

    c = CASES[name]
    pr = problem(c["problem"])
    kw = dict(c["kwargs"], d=pr["d"], Hdiag=pr["Hdiag"])
    if "Q" in pr:
        kw["Q"] = pr["Q"]
    if pr["conv"] is not None:
        kw["options"] = dict(kw.get("options") or {}, **_lib.filter_conventions(**pr["conv"]))
    return (pr["A"], pr["B"], pr["C"], pr["D"], pr.get("q"), pr["Z"], pr["y"]), kw


def blocks(pr):
    """The cotangents to compare."""
    return ("A_bar", "B_bar", "C_bar", "D_bar", "Q_bar" if "Q" in pr else "q_bar", "d_bar", "h_bar") + (("Z_bar",) if pr["want_Z"] else ())


def draw(pr, i, perturb=None):
    """Keyword arguments of gradient_reference.logp_and_gradient for draw i.  ``perturb``: (rng, rel) moves every entry of
    A, B, C, D by rel of its size, the sign at random (structural zeros stay zero)."""
    import oracle

    def per_draw(x, ndim):
        return x[i] if x.ndim == ndim + 1 else x

    kw = dict(A=pr["A"][i], B=pr["B"][i], C=pr["C"][i], D=pr["D"][i], Z=per_draw(pr["Z"], 2), y=pr["y"], d=pr["d"], Hdiag=pr["Hdiag"],
              want_Z=pr["want_Z"], conventions=None if pr["conv"] is None else oracle.FilterConventions(**pr["conv"]))
    if "Q" in pr:
        kw["Q"] = per_draw(pr["Q"], 2)
    else:
        kw["q"] = per_draw(pr["q"], 1)
    if perturb is not None:
        rng, rel = perturb
        for x in "ABCD":
            kw[x] = kw[x] * (1.0 + rel * rng.choice([-1.0, 1.0], kw[x].shape))
    return kw


@functools.lru_cache(maxsize=None)
def reference(problem_name):
    """{draw: dict(logp, *_bar)} of the "newton" formulation for the draws of the problem that have a reference (computed once,
    shared, never modified)."""
    pr = problem(problem_name)
    out = {}
    for i in pr["draws"]:
        out[i] = gradient_reference.logp_and_gradient(**draw(pr, i))
        for a in out[i].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out
