"""Autograd reference of the likelihood across dated structural breaks and of its gradient (TEST INFRASTRUCTURE ONLY; a helper, not
a test module): the chained filter of tests/segmented_filter_reference.py restated on torch float64 CPU tensors -- the loop body of
``gradient_reference.filter_logp`` generalised to ``a0``, ``P0``, ``shift`` and per-segment matrices -- differentiated by
torch.autograd, so that every ENTRY of every cotangent of the device's hand-derived reverse sweep has an independent value to be
held to (tests/test_gpu_segmented_gradient.py; tests/test_segmented_gradient_reference.py holds this module to
``segmented_filter_reference`` and to itself).  It shares no code with the device.

Leaves, per draw: T (S, m, m), R (S, m, k), q (S, k) or Q (S, k, k), Z (S, p, m), d (S, p), h (S, p), shift (S, m), a0 (m,), P0 (m, m).
``d``, ``h``, ``shift`` and ``a0`` that the case leaves out are leaves at zero (the gradient at 0).  A full Q enters as (Q + Q') / 2
and a given P0 as (P0 + P0') / 2: the gradient of the symmetric parametrisation, entry (i, j) being half the derivative along
E_ij + E_ji for i != j -- the convention of ``gradient_reference`` for ``Q_bar``.  Without a given P0 the initial covariance is the
stationary one of segment 0 (``lyapunov_kronecker``, or ``lyapunov_doubling`` as the second formulation) and ``P0_bar`` is zero.
Cotangents are per draw, also for inputs the draws share."""
import functools
import math

import numpy as np
import torch

import oracle
from oracle.statespace import JITTER_DEFAULT, MISSING_FILL

from tests import gradient_reference as GR
from tests import segmented_filter_cases as FC
from tests.segmented_filter_reference import segment_of

CPU = GR.CPU
_t = GR._t
_LN2PI = float(np.log(2.0 * np.pi))
LEAVES = ("T", "R", "q", "Z", "d", "h", "shift", "a0", "P0")


def _period(yt, a, P, Z, h, d, cv, jit_F, jit_P, missing_fill_value):
    """One measurement update: ``gradient_reference.filter_logp``'s loop body.  Returns (ll_t, a_filt, P_filt)."""
    m, p = P.shape[0], Z.shape[0]
    eye_m = torch.eye(m, dtype=torch.float64, device=CPU)
    eye_p = torch.eye(p, dtype=torch.float64, device=CPU)
    miss = np.isnan(yt) | (yt == missing_fill_value)
    keep = _t((~miss).astype(np.float64))
    W = torch.diag(keep)
    Zm = W @ Z
    Hm = W @ torch.diag(h)
    ym = _t(np.where(miss, 0.0, yt))
    v = ym - ((d * keep if cv.mask_d else d) + Zm @ a)
    PZt = P @ Zm.T
    F = Zm @ PZt + Hm + jit_F * eye_p
    K = torch.linalg.solve(F.T, PZt.T).T
    IKZ = eye_m - K @ Zm
    a_f = a + K @ v
    if cv.joseph:
        P_f = GR._sym_quad(IKZ, P) + GR._sym_quad(K, Hm) + jit_P * eye_m
    else:
        P_f = P - K @ F @ K.T
        P_f = 0.5 * (P_f + P_f.T) + jit_P * eye_m
    ll = torch.zeros((), dtype=torch.float64, device=CPU)
    if not miss.all():
        inner = v @ torch.linalg.solve(F, v)
        n_const = {"p": p, "observed": int((~miss).sum()), "one": 1}[cv.ll_constant]
        ll = -0.5 * (n_const * _LN2PI + torch.log(torch.linalg.det(F)) + inner)
    return ll, a_f, P_f


def segmented_logp(y, T, R, Q, Z, h, d, shift, a0, P0, seg_start, conventions=None, lyapunov="kronecker", jitter=JITTER_DEFAULT,
                   missing_fill_value=MISSING_FILL, per_period=False):
    """The chained filter on tensors: T (S, m, m) .. shift (S, m); Q (S, k, k) symmetric; P0 (m, m) or None.  Returns logp, or with
    ``per_period`` the list of its terms ll_t."""
    cv = oracle.DEFAULT_CONVENTIONS if conventions is None else conventions
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    jit_F = jitter if cv.jitter_on_F else 0.0
    jit_P = jitter if cv.jitter_on_P else 0.0
    RQR = [0.5 * (x + x.T) for x in (R[s] @ Q[s] @ R[s].T for s in range(T.shape[0]))]
    a = a0
    P = P0 if P0 is not None else {"kronecker": GR.lyapunov_kronecker, "doubling": GR.lyapunov_doubling}[lyapunov](T[0], R[0] @ Q[0] @ R[0].T)
    total, terms = torch.zeros((), dtype=torch.float64, device=CPU), []
    for t in range(y.shape[0]):
        s = segment_of(seg_start, t)
        ll, a_f, P_f = _period(y[t], a, P, Z[s], h[s], d[s], cv, jit_F, jit_P, missing_fill_value)
        total = total + ll
        terms.append(ll)
        if t + 1 < y.shape[0]:
            s2 = segment_of(seg_start, t + 1)
            if s2 != s:
                a_f = a_f + shift[s2]
            a = T[s2] @ a_f
            P = GR._sym_quad(T[s2], P_f) + RQR[s2]
    return terms if per_period else total


def _per_draw(x, b, shared_ndim, fill):
    if x is None:
        return fill
    x = np.asarray(x)
    return x if x.ndim == shared_ndim else x[b]


def draw_leaves(c, b, grad=True):
    """The leaf tensors of draw ``b`` of a case of tests/segmented_filter_cases.py, and whether its covariance is full."""
    S, m = c["T"].shape[1:3]
    p = c["y"].shape[1]
    full = c["q_mode"] in ("full", "full_batched")
    q = np.asarray(c["q"])
    q = q[b] if c["q_mode"] in ("diag_batched", "full_batched") else q
    vals = dict(T=c["T"][b], R=c["R"][b], q=q, Z=_per_draw(c["Z"], b, 3, None), d=_per_draw(c["d"], b, 2, np.zeros((S, p))),
                h=_per_draw(c["H"], b, 2, np.zeros((S, p))), shift=np.zeros((S, m)) if c["shift"] is None else c["shift"][b],
                a0=np.zeros(m) if c["a0"] is None else c["a0"][b], P0=None if c["P0"] is None else c["P0"][b])
    return {key: None if v is None else _t(v, grad) for key, v in vals.items()}, full


def logp_of_leaves(c, leaves, full, conventions=None, lyapunov="kronecker", per_period=False):
    Q = 0.5 * (leaves["q"] + leaves["q"].transpose(1, 2)) if full else torch.diag_embed(leaves["q"])
    P0 = None if leaves["P0"] is None else 0.5 * (leaves["P0"] + leaves["P0"].T)
    cv = None if conventions is None else oracle.FilterConventions(**conventions)
    return segmented_logp(c["y"], leaves["T"], leaves["R"], Q, leaves["Z"], leaves["h"], leaves["d"], leaves["shift"], leaves["a0"], P0,
                          c["seg_start"], conventions=cv, lyapunov=lyapunov, per_period=per_period)


def logp_and_gradient(c, b, conventions=None, lyapunov="kronecker"):
    """Draw ``b`` of case ``c``: dict(logp, T_bar, R_bar, q_bar | Q_bar, Z_bar, d_bar, h_bar, shift_bar, a0_bar, P0_bar) of numpy
    arrays in the device's per-draw layouts (shift_bar row 0 and, without a given P0, P0_bar are zero)."""
    leaves, full = draw_leaves(c, b)
    logp = logp_of_leaves(c, leaves, full, conventions, lyapunov)
    names = [key for key in LEAVES if leaves[key] is not None]
    grads = torch.autograd.grad(logp, [leaves[key] for key in names], allow_unused=True)
    out = {}
    for key, g in zip(names, grads):
        out[("Q_bar" if full else "q_bar") if key == "q" else key + "_bar"] = (torch.zeros_like(leaves[key]) if g is None else g).numpy().copy()
    if leaves["P0"] is None:
        out["P0_bar"] = np.zeros((c["T"].shape[2],) * 2)
    out["logp"] = float(logp.detach())
    return out


def reference(c, conventions=None, lyapunov="kronecker"):
    """draw -> ``logp_and_gradient``."""
    return {b: logp_and_gradient(c, b, conventions, lyapunov) for b in range(c["T"].shape[0])}


FD_LEVELS, FD_H0 = 6, 2.0 ** -6


def directional_derivative(c, b, key, direction, conventions=None):
    """d logp / d eps along ``direction`` in leaf ``key`` by central differences on the ladder h_k = h0 / 2^k (h0 = 2^-6 of the
    leaf's largest entry per unit of the direction's largest) with Romberg extrapolation, D[k][j] = (4^j D[k][j-1] - D[k-1][j-1]) /
    (4^j - 1): the entry whose two neighbours in its column agree best is returned, with that disagreement as its error estimate.
    The difference is taken PER PERIOD, sum_t (ll_t(x + h u) - ll_t(x - h u)) with an exact sum, so that the cancellation is that of
    one term of size ~ 10 and not of their total.  The value function is this module's without autograd, the stationary P0 by
    doubling (the Kronecker solve costs more than the filter).  Returns (derivative, estimate)."""
    leaves, full = draw_leaves(c, b, grad=False)
    u = _t(direction)
    x0 = leaves[key]
    top = float(x0.abs().max())
    h0 = FD_H0 * (top if top > 0.0 else 1.0) / float(u.abs().max())

    def terms(step):
        with torch.no_grad():
            return [float(x) for x in logp_of_leaves(c, {**leaves, key: x0 + step * u}, full, conventions, lyapunov="doubling",
                                                     per_period=True)]

    D = [[math.fsum(p - q for p, q in zip(terms(h), terms(-h))) / (2.0 * h)] for h in (h0 / 2.0 ** k for k in range(FD_LEVELS))]
    best, est = D[-1][0], np.inf
    for k in range(1, FD_LEVELS):
        for j in range(1, k + 1):
            D[k].append((4.0 ** j * D[k][j - 1] - D[k - 1][j - 1]) / (4.0 ** j - 1.0))
            if j < k and abs(D[k][j] - D[k - 1][j]) < est:
                best, est = D[k][j], abs(D[k][j] - D[k - 1][j])
    return best, est


# ---- the fused chain: A .. D -> T_s, R_s per segment (policy_newton), then the filter -----------------------------------------------
def fused_logp_and_gradient(A, B, C, D, c, b, conventions=None):
    """Draw ``b``: A, B, C (S, n, n), D (S, n, k) leaves; T_s by ``gradient_reference.policy_newton``, R_s = -(C_s T_s + B_s)^-1 D_s;
    every other input from case ``c`` (whose T, R are ignored).  Returns the dict of ``logp_and_gradient`` plus A_bar .. D_bar."""
    leaves, full = draw_leaves(c, b)
    abcd = [_t(x, True) for x in (A, B, C, D)]
    At, Bt, Ct, Dt = abcd
    S = At.shape[0]
    Ts = [GR.policy_newton(At[s], Bt[s], Ct[s]) for s in range(S)]
    Rs = [-torch.linalg.solve(Ct[s] @ Ts[s] + Bt[s], Dt[s]) for s in range(S)]
    T, R = torch.stack(Ts), torch.stack(Rs)
    T.retain_grad()
    R.retain_grad()
    logp = logp_of_leaves(c, {**leaves, "T": T, "R": R}, full, conventions)
    names = [key for key in LEAVES if key not in ("T", "R") and leaves[key] is not None]
    grads = torch.autograd.grad(logp, abcd + [T, R] + [leaves[key] for key in names], allow_unused=True)
    out = {key + "_bar": g.numpy().copy() for key, g in zip(("A", "B", "C", "D", "T", "R"), grads[:6])}
    for key, g in zip(names, grads[6:]):
        out[("Q_bar" if full else "q_bar") if key == "q" else key + "_bar"] = (torch.zeros_like(leaves[key]) if g is None else g).numpy().copy()
    if leaves["P0"] is None:
        out["P0_bar"] = np.zeros((T.shape[1],) * 2)
    out.update(logp=float(logp.detach()), T=T.detach().numpy().copy(), R=R.detach().numpy().copy())
    return out


# cases of the gradient's own, next to the accuracy cases of tests/segmented_filter_cases.py: name -> (builder, options of ``build``)
EXTRA_SPECS = {
    # a middle segment at rho(T) = 1.05 for two periods WITH P0 given (``explosive_middle`` of the filter's cases has the stationary P0)
    "explosive_middle_P0": ("sw17", dict(seg_start=(0, 3, 5), rho=(1, 1.05), P0=True)),
}
GRADIENT_CASES = tuple(FC.ACCURACY_CASES) + tuple(EXTRA_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in EXTRA_SPECS:
        builder, kw = EXTRA_SPECS[name]
        return FC.build(builder, **kw)
    return FC.case(name)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The reference of every draw of case ``name`` (computed once, shared, never modified)."""
    return reference(case(name))
