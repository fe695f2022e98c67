"""Inputs of the edge checks of the second-order path (TEST INFRASTRUCTURE ONLY; a helper, not a test module), as
tests/gradient_cases.py serves the gradient: tests/test_second_order_reference.py holds the oracle (oracle/second_order.py) to itself
on them, tests/test_gpu_second_order_edges.py the device to the oracle -- the same arrays, built once, read-only.

A PROBLEM is dict(A, B, C (nb, n, n), D (nb, n, k), idx (nnz, 3), val (nb, nnz), q (nb, k) | (k,), Z (p, n), y (T_len, p), d (p,) | None,
Hdiag (p,) | None).  ``reference(name)`` gives, per draw, what ``oracle.second_order.solve_second_order_logp`` returns plus the
dimensions m and u of the pruned state.

Unless its variant says otherwise a problem has 2 draws of ``workloads.sw_shaped_system(seed + i, n, s, n_lead, k)``, six Hessian
entries per equation with standard normal values, q uniform in [0.5e-4, 4e-4] per draw, H = 1e-5, d ~ N(0, 0.01), y ~ N(0, 0.02) over
24 steps with y[7, 0] missing and row 11 all missing; cycle reduction runs to 1e-13.

The design matrix of a shape with u - s observed non-states: row o loads on state o with a value of {1, 0.5, -2}; the non-states
(variables s .. u - 1) are dealt round-robin to the rows with values of {1, 0.25, -0.5}, so a row carries several loadings whenever
u - s > p.

SHAPES are the smallest that reach each edge of the kernels: m = 2 u + s (s + 1) / 2 on both sides of every boundary between two of the
five tile instances (2, 4, 7, 10, 13 tiles of 16) and at the entry's limit of 208; u > 24 (the second trip of the two-group P Z'
gather), u = 40, p = 1 and 8, k = s = 12 (234 rank-1 rows in Qz).

Every case has to pass tests/test_second_order_reference.py; one that does not is given another seed in SEEDS, never a wider bar."""
import functools

import numpy as np

from geconpy_amd import workloads as wl
from geconpy_amd.batched import MISSING_FILL
from oracle import second_order as so

T_LEN = 24
TOL = 1e-13
# name -> ((n, s, n_lead, k, p, u), m, tile instance)
SHAPES = {
    "m32": ((16, 4, 4, 2, 7, 11), 32, 2),
    "m33": ((16, 5, 4, 2, 4, 9), 33, 4),
    "m64": ((20, 8, 6, 3, 6, 14), 64, 4),
    "m65": ((20, 9, 6, 3, 1, 10), 65, 7),
    "m112": ((28, 12, 8, 4, 5, 17), 112, 7),
    "m113": ((36, 10, 8, 4, 8, 29), 113, 10),
    "m160": ((32, 15, 9, 5, 5, 20), 160, 10),
    "m161": ((36, 14, 9, 5, 8, 28), 161, 13),
    "m208": ((40, 16, 12, 6, 8, 36), 208, 13),
    "u40": ((44, 8, 10, 3, 8, 40), 116, 10),
    "k12": ((24, 12, 7, 12, 8, 12), 102, 7),
    "k_eq_s": ((12, 3, 3, 3, 2, 4), 14, 2),
}
VARIANTS = ("Hdiag_none", "d_none", "q_shared", "first_missing", "fill_marker", "tlen1", "tlen2")
VARIANT_BASES = ("m33", "m64")
# shapes the entry refuses (DSGE_ERR_INVALID); m = 210 and u = 41 are m208 and u40 with one more loading
REFUSED = {"k13": (28, 14, 8, 13, 2, 14), "p9": (20, 10, 6, 3, 9, 10), "k_gt_s": (12, 3, 3, 4, 2, 4)}
# nested models of m33 for the two neighbouring instances: the last observed non-state dropped (m = 31), one more loading (m = 35)
NESTED = {"m33_less": ("m33", -1, 31, 2), "m33_more": ("m33", +1, 35, 4)}
# case -> seed of its first draw.  Every seed was chosen so that the case passes tests/test_second_order_reference.py, above all the
# conditioning check: seeds taken at random move a coefficient block by 1.1e-10 .. 2e-9, and from n = 28 on an amplification below 10
# is rare -- the median draw of the generator moves a block by 4e-10 .. 6e-10.  The seeds of the large shapes are the consecutive pairs
# with the smallest cond(B + C T*) max(1, cond(B + C T* + C) / 10) among 3e4 (m208: 4e5, u40: 4e6) seeds that then pass the check
# itself (tools/second_order_case_seeds.py is that search).  So these are ATYPICALLY WELL-CONDITIONED draws: what a typical draw at
# n >= 28 does at these bars is not covered here (the fuzzer and the SW-shaped tests run typical draws).  k_eq_s besides: its draws
# reach the steady-state switch at steps 22 and 36 (a seed with a spectral radius of 0.90 reaches it at step 101 of 160, too late for
# the late-mask tests).  m208 besides: no near-cancelling logp (one rejected seed had |logp| = 26 under sum |ll_t| = 335).
SEEDS = {"m32": 6214, "m33": 6477, "m64": 6562, "m65": 6298, "m112": 50441, "m113": 34898, "m160": 59846, "m161": 33473, "m208": 424503,
         "u40": 4248422, "k12": 5324, "k_eq_s": 5313}
TILES = (2, 4, 7, 10, 13)


def so_tiles(m):
    """The tile instance the launcher takes for a pruned state of dimension m (launch_second_order.hip: so_tiles)."""
    need = (m + 15) // 16
    return next((mt for mt in TILES if need <= mt), 0)


def design(n, s, p, u, extra=0):
    """The design matrix described above for u - s + extra observed non-states."""
    Z = np.zeros((p, n))
    for o in range(p):
        Z[o, o % s] = (1.0, 0.5, -2.0)[o % 3]
    for j in range(u - s + extra):
        Z[j % p, s + j] = (1.0, 0.25, -0.5)[j % 3]
    return Z


def _base(base, T_len=T_LEN, extra=0):
    return build(SHAPES[base][0], SEEDS[base], T_len, extra)


def build(shape, seed, T_len=T_LEN, extra=0):
    """A problem of the shape (n, s, n_lead, k, p, u), with ``extra`` observed non-states more (or fewer) than u - s."""
    n, s, nl, k, p, u = shape
    rng = np.random.default_rng([31, seed])
    sysm = [wl.sw_shaped_system(seed + i, n, s, nl, k)[:4] for i in range(2)]
    A, B, C, D = (np.stack([s_[j] for s_ in sysm]) for j in range(4))
    idx = wl.second_order_hessian_pattern(A[0], C[0], k, nnz_per_eq=6, seed=seed)
    val = rng.standard_normal((2, len(idx)))
    q = rng.uniform(0.5e-4, 4e-4, (2, k))
    d = rng.normal(0, 0.01, p)
    y = rng.normal(0, 0.02, (T_len, p))
    if T_len > 11:
        y[7, 0] = np.nan
        y[11, :] = np.nan
    return dict(A=A, B=B, C=C, D=D, idx=idx, val=val, q=q, Z=design(n, s, p, u, extra), y=y, d=d, Hdiag=np.full(p, 1e-5))


def _freeze(pr):
    for a in pr.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def problem(name):
    if name in SHAPES:
        return _freeze(_base(name))
    if name in NESTED:
        return _freeze(_base(NESTED[name][0], extra=NESTED[name][1]))
    base, variant = name.split("_", 1)
    if base not in VARIANT_BASES or variant not in VARIANTS:
        raise KeyError(name)
    pr = _base(base)
    if variant == "Hdiag_none":
        pr["Hdiag"] = None
    elif variant == "d_none":
        pr["d"] = None
    elif variant == "q_shared":
        pr["q"] = pr["q"][0].copy()
    elif variant == "first_missing":
        pr["y"][0, :] = np.nan
    elif variant == "fill_marker":
        pr["y"][9, 0] = MISSING_FILL
    elif variant == "tlen1":
        pr["y"] = pr["y"][:1].copy()
    elif variant == "tlen2":
        pr["y"] = pr["y"][:2].copy()
        pr["y"][1, -1] = np.nan
    return _freeze(pr)


CASES = tuple(SHAPES) + tuple(f"{b}_{v}" for b in VARIANT_BASES for v in VARIANTS)
BLOCKS = ("g_yy", "g_yu", "g_uu", "g_ss")


def refused():
    """{name: (problem, the part of the entry's message that names the limit)} of the calls the entry refuses."""
    sizes = "sizes out of range"
    out = {"m210": (_base("m208", extra=1), "exceeds 208"), "u41": (_base("u40", extra=1), sizes)}
    out.update({name: (build(shape, 6100), "p out of range" if name == "p9" else sizes) for name, shape in REFUSED.items()})
    return out


def with_sample(pr, y):
    """The problem on another sample (not cached: the caller keeps it)."""
    return _freeze(dict(pr, y=np.array(y)))


def long_problem(base, T_len):
    """The model of a case with a complete panel of T_len steps (the steady-state tests)."""
    pr = _base(base, T_len=T_len)
    y = np.array(pr["y"])
    rng = np.random.default_rng([37, T_len])
    miss = np.isnan(y)
    y[miss] = rng.normal(0, 0.02, int(miss.sum()))
    return _freeze(dict(pr, y=y))


def draw(pr, i, perturb=None):
    """Keyword arguments of ``so.solve_second_order_logp`` for draw i.  ``perturb``: (rng, rel) moves every entry of A, B, C, D by rel
    of its size, the sign at random (structural zeros stay zero)."""
    q = pr["q"] if pr["q"].ndim == 1 else pr["q"][i]
    kw = dict(A=pr["A"][i], B=pr["B"][i], C=pr["C"][i], D=pr["D"][i], hess_idx=pr["idx"], hess_val=pr["val"][i], Sigma=np.diag(q), Z=pr["Z"],
              y=pr["y"], H=None if pr["Hdiag"] is None else np.diag(pr["Hdiag"]), d=pr["d"], tol=TOL)
    if perturb is not None:
        rng, rel = perturb
        for x in "ABCD":
            kw[x] = kw[x] * (1.0 + rel * rng.choice([-1.0, 1.0], kw[x].shape))
    return kw


def evaluate_reference(pr):
    """[per draw: dict(logp, T, R, sol, m, u)] of the oracle."""
    out = []
    for i in range(pr["A"].shape[0]):
        r = so.solve_second_order_logp(**draw(pr, i))
        assert r["sol"] is not None, "cycle reduction failed in the oracle"
        S = np.asarray(r["sol"]["S"])
        u = len(so.retained_variables(S, np.flatnonzero((pr["Z"] != 0).any(axis=0))))
        r.update(u=u, m=2 * u + len(S) * (len(S) + 1) // 2)
        for a in r["sol"].values():
            a.setflags(write=False)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle on a named problem (computed once, shared, never modified)."""
    return evaluate_reference(problem(name))


def entry_point_arguments(pr):
    """(positional, keyword) arguments of ``batched.second_order_logp_batched``."""
    return (pr["A"], pr["B"], pr["C"], pr["D"], pr["idx"], pr["val"], pr["q"], pr["Z"], pr["y"]), dict(d=pr["d"], Hdiag=pr["Hdiag"], tol=TOL)
