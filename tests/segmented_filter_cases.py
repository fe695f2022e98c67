"""Inputs of the segmented filter's tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the same arrays, built once and
read-only, for tests/test_segmented_filter_reference.py (numpy forms against each other) and tests/test_gpu_segmented_filter.py
(the device against the reference).

Segments are built from ``sw_model`` / ``dense_model`` of tests/smoother_cases.py: segment s of draw b is the builder's draw
(b + s) mod nb, its shock variances scaled by 1, 4, 0.25 (cyclically), d = 0.01 s, H = H0 (1 + s), Z scaled by 1 + s / 16 (so that a
boundary that forgot to re-stage Z shows).  Unless a case says otherwise: 2 draws, 8 periods simulated from draw 0, S = 3 with breaks at
t = 3 and t = 6, y[2, 0] missing, Q diagonal per draw, Z / d / H shared by the draws, no shift, a0 or P0.

A case is dict(T (nb, S, m, m), R (nb, S, m, k), q, q_mode, Z, d, H, y, seg_start, a0, P0, shift, conv); ``draw(c, b)`` gives the
list of per-segment matrices of one draw as tests/segmented_filter_reference.py takes them, ``reference(name)`` the reference of
every draw (computed once, shared, never modified)."""
import functools
import itertools

import numpy as np

import oracle

from tests import smoother_cases as SC
from tests.segmented_filter_reference import innovation_conditions, segmented_filter

N_STEPS, H0 = 8, 1e-5
Q_SCALE = (1.0, 4.0, 0.25)
COND_MAX = 1e4

# builder -> what it is: every edge of the 16-row tiles and of the LDS budget, p in {1, 4, 16}, k = 1 and k = m
BUILDERS = ("dense1", "dense2", "zc16", "sw17", "dense32", "dense33", "dense48", "zc49", "dense64", "dense64_p16", "dense20_k20",
            "dense64_k64")
# (m, k, p) of a builder for the tests that hold the device against itself: no case of ``SPECS``, no reference
SMALL = {"dense5": (5, 2, 2)}

# name -> (builder, options of ``build``)
SPECS = {f"size_{b}": (b, {}) for b in BUILDERS}
SPECS.update({
    "s1": ("sw17", dict(seg_start=(0,))),
    "s8": ("sw17", dict(seg_start=tuple(range(8)))),
    "one_period": ("sw17", dict(seg_start=(0,), n=1)),
    "two_periods_two_segments": ("dense33", dict(seg_start=(0, 1), n=2, shift=True)),
    "break_first": ("sw17", dict(seg_start=(0, 1))),
    "break_last": ("sw17", dict(seg_start=(0, N_STEPS - 1))),
    "miss_entry_at_boundary": ("sw17", dict(missing=((3, 1),))),
    "miss_period_at_boundary": ("sw17", dict(missing=((3, 0), (3, 1), (3, 2), (3, 3)))),
    "complete": ("sw17", dict(missing=())),
    "fill_marker_at_boundary": ("sw17", dict(missing=(), fill=((6, 2),))),
    "q_diag": ("dense33", dict(q_mode="diag")),
    "q_diag_batched": ("dense33", dict(q_mode="diag_batched")),
    "q_full": ("dense33", dict(q_mode="full")),
    "q_full_batched": ("dense33", dict(q_mode="full_batched")),
    "zero_shock_one_segment": ("sw17", dict(zero_shock=(1, 1))),  # (segment, shock)
    "obs_batched": ("sw17", dict(nb=3, obs_batched=True)),
    "obs_null": ("dense16", dict(obs_null=True)),
    "shift": ("sw17", dict(shift=True)),
    "a0": ("sw17", dict(a0=True)),
    "P0": ("sw17", dict(P0=True)),
    "shift_a0_P0": ("dense33", dict(shift=True, a0=True, P0=True)),
    "explosive_middle": ("sw17", dict(seg_start=(0, 3, 5), rho=(1, 1.05))),  # (segment, spectral radius)
})
ACCURACY_CASES = tuple(SPECS)
CONVENTIONS = tuple(dict(ll_constant=lc, jitter_on_F=jf, jitter_on_P=jp, mask_d=md, joseph=jo)
                    for lc, jf, jp, md, jo in itertools.product(("p", "observed", "one"), *[(True, False)] * 4))
CONVENTION_CASE_COMPLETE = "complete"  # the same panel with nothing missing
CONVENTION_CASE = "miss_entry_at_boundary"  # 17 variables, y[3, 1] missing: the first period of segment 1, where d != 0


def _base(builder, nb, rng):
    if builder == "sw17" or builder in SC.ZERO_COLUMN:
        shape = SC.SW17 if builder == "sw17" else SC.ZERO_COLUMN[builder][0]
        T, R, sigma = SC.sw_model(nb, shape)
        return T, R, sigma, np.eye(4, shape[0])
    m, k, p = SMALL[builder] if builder in SMALL else SC.DENSE[builder]
    return SC.dense_model(nb, m, k, p, rng)


def build(builder, nb=2, seg_start=(0, 3, 6), n=N_STEPS, q_mode="diag_batched", missing=((2, 0),), fill=(), zero_shock=None,
          obs_batched=False, obs_null=False, shift=False, a0=False, P0=False, rho=None):
    rng = np.random.default_rng([29, *builder.encode()])
    T0, R0, sigma, Z0 = _base(builder, nb, rng)
    S, (m, k), p = len(seg_start), R0.shape[1:], Z0.shape[0]
    pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % nb  # segment s of draw b: the builder's draw (b + s) mod nb
    T, R = T0[pick].copy(), R0[pick].copy()
    qs = np.array([Q_SCALE[s % 3] for s in range(S)])
    if rho is not None:
        s, r = rho
        for b in range(nb):
            T[b, s] *= r / np.abs(np.linalg.eigvals(T[b, s])).max()
    if q_mode in ("diag", "diag_batched"):
        q = (sigma[pick] ** 2 * qs[None, :, None]) if q_mode == "diag_batched" else sigma[np.arange(S) % nb] ** 2 * qs[:, None]
        if zero_shock is not None:
            q[..., zero_shock[0], zero_shock[1]] = 0.0
    else:
        full = lambda i, s: (lambda L: L @ L.T * qs[s])(SC.chol_factor(sigma[i], rng))  # noqa: E731
        q = (np.stack([np.stack([full(pick[b, s], s) for s in range(S)]) for b in range(nb)]) if q_mode == "full_batched"
             else np.stack([full(s % nb, s) for s in range(S)]))
    zs = 1.0 + np.arange(S) / 16.0
    Z = Z0[None] * zs[:, None, None]
    d = 0.01 * np.arange(S)[:, None] * np.ones(p)
    H = H0 * (1.0 + np.arange(S))[:, None] * np.ones(p)
    if obs_batched:
        sc = 1.0 + np.arange(nb) / 16.0
        Z = Z[None] * sc[:, None, None, None]
        d = d[None] + 0.003 * np.arange(nb)[:, None, None]
        H = H[None] * sc[:, None, None] ** 2
    if obs_null:
        d = H = None
    c = dict(T=T, R=R, q=q, q_mode=q_mode, Z=Z, d=d, H=H, seg_start=tuple(int(x) for x in seg_start), conv=None,
             shift=0.01 * rng.standard_normal((nb, S, m)) if shift else None, a0=0.01 * rng.standard_normal((nb, m)) if a0 else None,
             P0=None)
    if P0:  # one and a half times the stationary covariance of segment 0, plus a ridge: symmetric positive definite, not the default
        c["P0"] = np.stack([1.5 * oracle.solve_discrete_lyapunov(x["T"], x["R"] @ x["Q"] @ x["R"].T) + 1e-4 * np.eye(m)
                            for x in (draw(c, b)[0] for b in range(nb))])
        c["P0"] = 0.5 * (c["P0"] + c["P0"].transpose(0, 2, 1))
    c["y"] = simulate(c, n, rng)
    for t, o in missing:
        if t < n and o < p:
            c["y"][t, o] = np.nan
    for t, o in fill:
        c["y"][t, o] = oracle.MISSING_FILL
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def q_full(c, b, s):
    q, mode = c["q"], c["q_mode"]
    q = q[b, s] if mode in ("diag_batched", "full_batched") else q[s]
    return np.diag(q) if mode in ("diag", "diag_batched") else np.array(q)


def _seg_slice(x, b, s, shared_ndim):
    """Segment s of an array shared by the draws (``shared_ndim`` axes) or with a leading draw axis; None stays None."""
    if x is None:
        return None
    return x[s] if x.ndim == shared_ndim else x[b, s]


def draw(c, b):
    """The per-segment matrices of draw b: a list of dict(T, R, Q (k, k), Z (p, m), d (p,) or None, H (p, p) or None)."""
    S = c["T"].shape[1]
    out = []
    for s in range(S):
        Hs = _seg_slice(c["H"], b, s, 2)
        out.append(dict(T=c["T"][b, s], R=c["R"][b, s], Q=q_full(c, b, s), Z=_seg_slice(c["Z"], b, s, 3), d=_seg_slice(c["d"], b, s, 2),
                        H=None if Hs is None else np.diag(Hs)))
    return out


def simulate(c, n, rng):
    """A panel of n periods from draw 0, the matrices switching at the breaks."""
    segs, starts = draw(c, 0), np.asarray(c["seg_start"])
    m = segs[0]["T"].shape[0]
    x = np.zeros(m)
    y = np.empty((n, segs[0]["Z"].shape[0]))
    for t in range(n):
        g = segs[int(np.searchsorted(starts, t, side="right") - 1)]
        w, v = np.linalg.eigh(g["Q"])
        x = g["T"] @ x + g["R"] @ ((v * np.sqrt(np.clip(w, 0.0, None))) @ rng.standard_normal(g["Q"].shape[0]))
        noise = 0.0 if g["H"] is None else rng.standard_normal(y.shape[1]) * np.sqrt(np.diag(g["H"]))
        y[t] = g["Z"] @ x + (0.0 if g["d"] is None else g["d"]) + noise
    return y


@functools.lru_cache(maxsize=None)
def case(name):
    builder, kw = SPECS[name]
    return build(builder, **kw)


def reference_of(c, conventions=None):
    """draw -> the reference's dict, for the arrays of case dict ``c``."""
    cv = None if conventions is None else oracle.FilterConventions(**conventions)
    out = {}
    for b in range(c["T"].shape[0]):
        out[b] = segmented_filter(c["y"], draw(c, b), c["seg_start"], a0=None if c["a0"] is None else c["a0"][b],
                                  P0=None if c["P0"] is None else c["P0"][b], shift=None if c["shift"] is None else c["shift"][b],
                                  conventions=cv)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(case(name))


def check_conditions(name):
    """From the reference alone: finite logp and cond_2(F_t) <= COND_MAX at every period of every draw.  Returns the largest cond."""
    c, worst = case(name), 0.0
    for b, res in reference(name).items():
        assert np.isfinite(res["logp"]) and np.isfinite(res["ll"]).all(), (name, b)
        worst = max(worst, innovation_conditions(c["y"], draw(c, b), c["seg_start"], res).max())
    assert worst <= COND_MAX, (name, worst)
    return worst
