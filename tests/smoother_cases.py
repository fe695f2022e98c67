"""Inputs of the smoother's edge cases (TEST INFRASTRUCTURE ONLY; a helper, not a test module): tests/test_smoother_reference.py
holds the two numpy forms of the recursion to each other on them, tests/test_gpu_smoother.py the device to the reference -- the
same arrays, built once, read-only.

A case is dict(T (nb, m, m), R (nb, m, k), q: the shock covariance AS PASSED to the device in layout ``q_mode``, Z (p, m) or
(nb, p, m), d None / (p,) / (nb, p), H (p,) or (nb, p), y (n, p), conv: FilterConventions keywords or None, r: expected rank of
[T | R_J], draws: the draws that have a reference).  ``draw(c, i)`` gives the matrices of one draw as the oracle takes them.

Unless its builder says otherwise a case has 2 draws, 8 steps simulated from draw 0, y[2, 0] missing and H = 1e-5."""
import functools

import numpy as np

import oracle
from geconpy_amd import workloads as wl

from tests.smoother_reference import rts_smoother

N_STEPS, H0 = 8, 1e-5
SW17 = (17, 7, 5, 3)

# zero-column models at the boundaries of the backward kernel's LDS classes (m <= 16, <= 32, 33..48, >= 49: U, U'T, U'R in global
# memory): (n, n_state, n_lead, k) -> r
ZERO_COLUMN = {"zc16": ((16, 7, 5, 3), 10), "zc32": ((32, 14, 10, 5), 19), "zc33": ((33, 14, 10, 5), 19),
               "zc48": ((48, 22, 14, 7), 29), "zc49": ((49, 22, 15, 7), 29)}
# dense T with [T | R] of full rank: r = m, the plain Rauch-Tung-Striebel case; (m, k, p)
DENSE = {"dense1": (1, 1, 1), "dense2": (2, 1, 1), "dense16": (16, 3, 2), "dense32": (32, 5, 4), "dense33": (33, 5, 4),
         "dense48": (48, 8, 4), "dense49": (49, 8, 4), "dense64": (64, 8, 4), "dense64_p16": (64, 8, 16), "dense20_k20": (20, 20, 3),
         "dense64_k64": (64, 64, 16)}
Q_FORMS = ("qfull", "qfull_batched", "qdiag_zero", "qfull_zero")
ZERO_SHOCK = 1  # the shock without variance in the *_zero forms
SHOCK_FORMS = {f"{base}_{form}": (base, form) for base in ("sw17", "dense33") for form in Q_FORMS}
OTHERS = ("obs_batched", "p1", "tlen2", "tlen3", "singular_m")

PARITY_CASES = tuple(ZERO_COLUMN) + tuple(DENSE) + tuple(SHOCK_FORMS) + OTHERS  # status 0 everywhere, every draw has a reference
ALL_CASES = PARITY_CASES + ("singular_m_nojit", "forward_fail")  # (these two: the reference of draws 0 and 2 only)


def sw_model(nb, shape):
    n, n_state, n_lead, k = shape
    b = wl.sw_shaped_batch(nb, n=n, n_state=n_state, n_lead=n_lead, k=k)
    T = b["T_star"]
    R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(nb)])
    return T, R, b["sigma"]


def dense_model(nb, m, k, p, rng):
    T = np.empty((nb, m, m))
    for i in range(nb):
        G = np.linalg.qr(rng.standard_normal((m, m)))[0]
        T[i] = 0.7 * G + 0.1 * rng.standard_normal((m, m)) / np.sqrt(m)
        assert np.abs(np.linalg.eigvals(T[i])).max() < 0.95
    R = rng.standard_normal((nb, m, k)) / np.sqrt(m)
    sigma = rng.uniform(0.005, 0.02, (nb, k))
    Z = rng.standard_normal((p, m)) * (rng.random((p, m)) < 0.3)
    Z[np.arange(p), np.arange(p)] = 1.0
    return T, R, sigma, Z


def chol_factor(sigma, rng):
    """L of a full Q = L L': diag(sigma) + 0.25 tril(N, -1) mean(sigma)."""
    k = sigma.shape[0]
    return np.diag(sigma) + 0.25 * np.tril(rng.standard_normal((k, k)), -1) * sigma.mean()


def _shock_form(form, sigma, rng):
    """(q, q_mode) of one of Q_FORMS from the per-draw standard deviations sigma (nb, k)."""
    nb = sigma.shape[0]
    if form == "qfull":
        L = chol_factor(sigma[0], rng)
        return L @ L.T, "full"
    if form == "qfull_batched":
        Ls = [chol_factor(sigma[i], rng) for i in range(nb)]
        return np.stack([L @ L.T for L in Ls]), "full_batched"
    if form == "qdiag_zero":
        q = sigma ** 2
        q[:, ZERO_SHOCK] = 0.0
        return q, "diag_batched"
    if form == "qfull_zero":
        Ls = [chol_factor(sigma[i], rng) for i in range(nb)]
        for L in Ls:
            L[ZERO_SHOCK, :] = 0.0
            L[:, ZERO_SHOCK] = 0.0
        return np.stack([L @ L.T for L in Ls]), "full_batched"
    raise KeyError(form)


def q_full(c, i):
    """The (k, k) shock covariance of draw i."""
    q, mode = c["q"], c["q_mode"]
    if mode in ("diag_batched", "full_batched"):
        q = q[i]
    return np.diag(q) if mode in ("diag", "diag_batched") else np.array(q)


def draw(c, i):
    """dict(T, R, Q (k, k), Z (p, m), d (p,) or None, H (p, p)) of draw i, as oracle.kalman_filter_logp takes them."""
    Z = c["Z"][i] if c["Z"].ndim == 3 else c["Z"]
    d = None if c["d"] is None else (c["d"][i] if c["d"].ndim == 2 else c["d"])
    H = c["H"][i] if c["H"].ndim == 2 else c["H"]
    return dict(T=c["T"][i], R=c["R"][i], Q=q_full(c, i), Z=Z, d=d, H=np.diag(H))


def simulate(c, n, rng):
    """A panel of n steps from draw 0 of the case."""
    d0 = draw(c, 0)
    w, v = np.linalg.eigh(d0["Q"])
    S = v * np.sqrt(np.clip(w, 0.0, None))  # Q = S S'  (Q may be singular)
    m, k = d0["R"].shape
    p = d0["Z"].shape[0]
    x = np.zeros(m)
    y = np.empty((n, p))
    for t in range(n):
        x = d0["T"] @ x + d0["R"] @ (S @ rng.standard_normal(k))
        y[t] = d0["Z"] @ x + (0.0 if d0["d"] is None else d0["d"]) + rng.standard_normal(p) * np.sqrt(np.diag(d0["H"]))
    return y


def _finish(c, rng, n=N_STEPS, missing=True):
    c.setdefault("d", None)
    c.setdefault("conv", None)
    c.setdefault("draws", tuple(range(c["T"].shape[0])))
    if "y" not in c:
        c["y"] = simulate(c, n, rng)
        if missing and n > 2:
            c["y"][2, 0] = np.nan
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng([17, *name.encode()])
    if name in ZERO_COLUMN:
        shape, r = ZERO_COLUMN[name]
        T, R, sigma = sw_model(2, shape)
        return _finish(dict(T=T, R=R, q=sigma ** 2, q_mode="diag_batched", Z=np.eye(4, shape[0]), H=np.full(4, H0), r=r), rng)
    if name in DENSE:
        m, k, p = DENSE[name]
        T, R, sigma, Z = dense_model(2, m, k, p, rng)
        return _finish(dict(T=T, R=R, q=sigma ** 2, q_mode="diag_batched", Z=Z, H=np.full(p, H0), r=m), rng)
    if name in SHOCK_FORMS:
        base, form = SHOCK_FORMS[name]
        if base == "sw17":
            T, R, sigma = sw_model(2, SW17)
            Z, r = np.eye(4, 17), 9 if form.endswith("_zero") else 10
        else:
            m, k, p = DENSE[base]
            T, R, sigma, Z = dense_model(2, m, k, p, rng)
            r = m
        q, q_mode = _shock_form(form, sigma, rng)
        return _finish(dict(T=T, R=R, q=q, q_mode=q_mode, Z=Z, H=np.full(Z.shape[0], H0), r=r,
                            zero_shock=ZERO_SHOCK if form.endswith("_zero") else None), rng)
    if name == "obs_batched":
        # Z, d, Hdiag and a full Q per draw, built as tests/test_gpu_smoother.py::test_chunked_equals_unchunked_every_member_batched
        # builds them (there the device is held to itself; here to the reference)
        T, R, s = sw_model(3, SW17)
        scale = 1.0 + np.arange(3) / 16.0
        Z = np.eye(4, 17)[None] * scale[:, None, None]
        d = np.random.default_rng(8).normal(0, 0.01, (3, 4))
        H = np.full(4, H0)[None] * scale[:, None] ** 2
        Q = np.stack([np.diag(s[i] ** 2) + 0.1 * scale[i] * (np.outer(s[i], s[i]) - np.diag(s[i] ** 2)) for i in range(3)])
        return _finish(dict(T=T, R=R, q=Q, q_mode="full_batched", Z=Z, d=d, H=H, r=10), rng)
    if name in ("p1", "tlen2", "tlen3"):
        T, R, sigma = sw_model(2, SW17)
        p = 1 if name == "p1" else 4
        n = {"p1": N_STEPS, "tlen2": 2, "tlen3": 3}[name]
        return _finish(dict(T=T, R=R, q=sigma ** 2, q_mode="diag_batched", Z=np.eye(p, 17), H=np.full(p, H0), r=10), rng, n=n)
    if name in ("singular_m", "singular_m_nojit"):
        # draw 1: the second variable has no shock and no link to the first, so its predicted variance and both off-diagonals are
        # exactly 0 at every step; without the P jitter the second pivot of M is exactly 0 (DSGE_ST_SMOOTHER_SINGULAR), with it M is
        # diag(1.3, 2.5e-9) and both forms invert it exactly.  Draws 0 and 2: the shock reaches both variables and T couples them
        # ([R, T R] has rank 2), so P_pred is well conditioned.  [With T = diag(0.5, 0.5) in these two as well, x_2 = x_1 / 2 exactly:
        # P_pred has rank 1 up to rounding, the second pivot of M is +-1e-17 without the P jitter, and with it the pinv form and the
        # range form differ by 8e-9 on the shocks -- inputs that decide nothing.]
        T = np.stack([np.array([[0.5, 0.0], [0.3, 0.4]]), np.diag([0.5, 0.5]), np.array([[0.5, 0.0], [0.3, 0.4]])])
        R = np.array([[[1.0], [0.5]], [[1.0], [0.0]], [[1.0], [0.5]]])
        nojit = name == "singular_m_nojit"
        return _finish(dict(T=T, R=R, q=np.array([1.0]), q_mode="diag", Z=np.array([[1.0, 0.0]]), H=np.array([0.01]), r=2,
                            y=np.random.default_rng(12).standard_normal((6, 1)), conv=dict(jitter_on_P=False) if nojit else None,
                            draws=(0, 2) if nojit else (0, 1, 2)), rng)
    if name == "forward_fail":
        # draw 1: the second row of Z is zero and its measurement error too, so without the F jitter F[1, 1] is exactly 0
        T, R, sigma = sw_model(3, SW17)
        Z = np.stack([np.eye(2, 17)] * 3)
        Z[1, 1] = 0.0
        return _finish(dict(T=T, R=R, q=sigma ** 2, q_mode="diag_batched", Z=Z, H=np.array([H0, 0.0]), r=10,
                            conv=dict(jitter_on_F=False), draws=(0, 2)), rng, missing=False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per draw of ``case(name)["draws"]``: (ll per step, the filter's states dict, smoothed states, covariances, shocks) from
    oracle.kalman_filter_logp(return_states=True) and rts_smoother (computed once, shared, never modified)."""
    c = case(name)
    cv = None if c["conv"] is None else oracle.FilterConventions(**c["conv"])
    out = {}
    for i in c["draws"]:
        x = draw(c, i)
        _, ll, stt = oracle.kalman_filter_logp(c["y"], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], return_states=True,
                                               conventions=cv)
        out[i] = (ll, stt) + rts_smoother(stt, x["T"], x["R"], x["Q"])
    return out


def scales(c, i, stt):
    """The scales of the 1e-9 bar (tests/test_gpu_smoother.py): states, covariances, shocks."""
    return max(1.0, np.abs(stt["a_filt"]).max()), np.abs(stt["P_pred"]).max(), np.sqrt(np.diag(q_full(c, i))).max()
