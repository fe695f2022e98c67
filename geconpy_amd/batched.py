"""Batched numpy front-end of the HIP engine (host arrays in, host arrays out).

Every function takes arrays with a leading draw axis, calls ONE C-ABI entry point of
libdsge_hip.so (the ``*_host`` twins, which stage through device memory) and returns fresh
numpy arrays.  Layout/dtype coercion mirrors the reference
(``np.ascontiguousarray(..., float64)``, gEconpy/solvers/gensys.py:625-628).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _frontend as F
from . import _lib
from ._frontend import HOST
from ._lib import DsgeHipError  # noqa: F401

JITTER_DEFAULT = 1e-8  # float64 cov_jitter default (gEconpy/model/statespace.py:22,1144)
MISSING_FILL = -9999.0  # default missing_fill_value (gEconpy/model/statespace.py:1143)
FILTER_TYPES_UPSTREAM = ("standard", "univariate", "steady_state", "single", "cholesky")


def check_filter_type(filter_type):
    """``filter_type`` of ``statespace_from_gcn`` / ``DSGEStateSpace`` (gEconpy/model/build.py:577, 608-609; statespace.py:69, 187:
    handed to PyMCStateSpace).  The device computes the log-likelihood of the "standard" filter -- the default, and the only one
    the oracle restates.  The other variants are different algorithms with their own jitter and missing-data conventions
    (univariate: observation-at-a-time updates; steady_state: a constant gain from the first step; single / cholesky: other
    factorisations of F); silently running the standard recursion under their name would return a number that differs from the
    reference's, so anything but "standard" raises."""
    if filter_type == "standard":
        return
    if filter_type in FILTER_TYPES_UPSTREAM:
        raise NotImplementedError(
            f"filter_type={filter_type!r}: only the 'standard' Kalman filter is built on the device "
            "(DESIGN.md section 7); evaluate this model with the reference's CPU filter")
    raise ValueError(f"unknown filter_type {filter_type!r}; upstream knows {FILTER_TYPES_UPSTREAM}")


def _f64(x, ndim=None):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise ValueError(f"expected a {ndim}-d array, got shape {a.shape}")
    return a


_ptr = HOST.ptr


def _check_abc(A, B, C):
    return F.check_abc(HOST, A, B, C)


def cycle_reduction_batched(A, B, C, max_iter=1000, tol=1e-9, options=None):
    """T, status, n_iter for a batch of systems (``_cycle_reduction_core`` semantics,
    gEconpy/solvers/cycle_reduction.py:127-183; Op defaults :190)."""
    A, B, C = _check_abc(A, B, C)
    nb, n, _ = A.shape
    T = np.empty_like(A)
    status = np.empty(nb, dtype=np.int32)
    n_iter = np.empty(nb, dtype=np.int32)
    with _lib.options_scope(options):
        _lib.check(
            _lib.load().dsge_cycle_reduction_batched_host(
                _ptr(A), _ptr(B), _ptr(C), nb, n, int(max_iter), float(tol), _ptr(T), _ptr(status), _ptr(n_iter)
            )
        )
    return T, status, n_iter


def scan_cycle_reduction_batched(A, B, C, max_iter=50, tol=1e-7):
    """Batched ``scan_cycle_reduction`` (gEconpy/solvers/cycle_reduction.py:246-325) -> (T, status, n_steps):
    A0-norm-only stopping rule, fixed trip count, 1e-16 diagonal jitter in every solve."""
    A, B, C = _check_abc(A, B, C)
    nb, n, _ = A.shape
    T = np.empty_like(A)
    status = np.empty(nb, dtype=np.int32)
    n_steps = np.empty(nb, dtype=np.int32)
    _lib.check(
        _lib.load().dsge_scan_cycle_reduction_batched_host(_ptr(A), _ptr(B), _ptr(C), nb, n, int(max_iter), float(tol),
                                                           _ptr(T), _ptr(status), _ptr(n_steps))
    )
    return T, status, n_steps


def lead_hint(C, tol=0.0):
    """Performance hint: number of columns of ``C`` (any leading batch axes) whose absolute column
    sum exceeds ``tol`` in at least one draw -- the forward-looking variables (gensys.py:580-589)."""
    C = np.asarray(C)
    cs = np.abs(C).sum(axis=-2)
    return int(np.count_nonzero(np.any(cs.reshape(-1, C.shape[-1]) > tol, axis=0)))


def gensys_batched(A, B, C, D=None, tol=1e-8, n_lead_hint=None, options=None):
    """Batched ``GensysWrapper`` / ``gensys_pt`` (gEconpy/solvers/gensys.py:634-683):
    returns dict(T, success, eu, status[, R]).

    ``eu[i]`` is the reference's code triple -- with ONE code the reference does not have: for 65 .. 96 variables (no ordered QZ at
    that size) a draw that the spectral-division certificate cannot prove regular comes back as ``eu = [-3, -3, 0]``
    (``_lib.EU_NO_VERDICT``), ``success = False``, ``T = R = 0``: "no verdict at this size", never a wrong one.  It covers non-regular
    draws (the reference would say ``[1, 0, k]``, ``[0, 1, 0]``, ...) AND regular ones with a root within 2e-4 of the unit circle
    or a scale defect (the reference would solve them); consumers written against ``interpret_gensys_output`` should treat it as a
    failed draw."""
    A, B, C = _check_abc(A, B, C)
    nb, n, _ = A.shape
    T = np.empty_like(A)
    eu = np.empty((nb, 3), dtype=np.int32)
    status = np.empty(nb, dtype=np.int32)
    R = None
    k = 1
    if D is not None:
        D = _f64(D, 3)
        k = D.shape[2]
        R = np.empty((nb, n, k))
    nl = lead_hint(C, tol) if n_lead_hint is None else int(n_lead_hint)
    with _lib.options_scope(options):
        _lib.check(
            _lib.load().dsge_gensys_batched_host(_ptr(A), _ptr(B), _ptr(C), _ptr(D), nb, n, k, float(tol), nl, _ptr(T),
                                                 _ptr(R), _ptr(eu), _ptr(status))
        )
    out = dict(T=T, success=status == 0, eu=eu, status=status)
    if R is not None:
        out["R"] = R
    return out


def gensys_pencil_batched(g0, g1, psi, pi, c=None, tol=1e-8, forward=False):
    """Batched ``gensys(g0, g1, c, psi, pi)`` (gEconpy/solvers/gensys.py:398-521) on caller-supplied pencils:
    returns dict(G1, C, impact, gev (batch, N, 2) complex (alpha, beta), eu, status, success).

    ``forward=True`` adds the forward-solution part of the reference's 9-tuple (:367-393), formed on the device by
    ``dsge_gensys_pencil_full_batched``: ``n_unstable`` (batch,) and, full-size with the valid block leading (slice with
    ``n_unstable[i]``), ``f_mat`` (batch, N, N) complex, ``f_wt`` (batch, N, k) complex, ``y_wt`` (batch, N, N) complex and
    ``loose`` (batch, N, n_eta).  When the columns of some ``pi[i]`` are not orthonormal two launches run (matrices from Pi as
    given, existence / uniqueness codes from an orthonormal basis of its column space; see the comment below)."""
    g0, g1 = _f64(g0, 3), _f64(g1, 3)
    psi, pi = _f64(psi, 3), _f64(pi, 3)
    nb, N, _ = g0.shape
    if g1.shape != (nb, N, N) or psi.shape[:2] != (nb, N) or pi.shape[:2] != (nb, N):
        raise ValueError("g0, g1: (batch, N, N); psi: (batch, N, k); pi: (batch, N, n_eta)")
    k, ne = psi.shape[2], pi.shape[2]
    if c is not None:
        c = _f64(c).reshape(nb, N)
    G1 = np.empty_like(g0)
    Cc = np.empty((nb, N))
    impact = np.empty((nb, N, k))
    gev = np.empty((nb, N, 4))
    eu = np.empty((nb, 3), dtype=np.int32)
    status = np.empty(nb, dtype=np.int32)
    lib = _lib.load()

    def call(fw):
        _lib.check(lib.dsge_gensys_pencil_full_batched_host(_ptr(g0), _ptr(g1), _ptr(c), _ptr(psi), _ptr(pi), nb, N, k, ne,
                                                            float(tol), _ptr(G1), _ptr(Cc), _ptr(impact), _ptr(gev),
                                                            _ptr(eu), _ptr(status),
                                                            None if fw is None else ctypes.addressof(fw)))

    # Pi with orthonormal columns (every gEconpy pencil: [0; I], gensys.py:606-611): one launch, Pi as given.  Any other Pi: the
    # matrices come from a launch on Pi AS GIVEN (for a non-unique solution G1, impact and loose depend on Pi itself, not only on
    # its column space: Phi = (Q1 Pi)(Q2 Pi)^+), the existence / uniqueness codes from a launch on an orthonormal basis of its
    # column space (they are rank decisions, which the device takes with orthonormal columns; include/dsge_hip.h).
    gram = np.einsum("bij,bik->bjk", pi, pi)
    orthonormal = ne == 0 or bool(np.abs(gram - np.eye(ne)).max() <= 1e-14)
    out = {}
    fw = None
    if forward:
        f_mat, y_wt = np.zeros((nb, N, N, 2)), np.zeros((nb, N, N, 2))
        f_wt = np.zeros((nb, N, k, 2))
        loose = np.zeros((nb, N, max(ne, 1)))
        n_unst = np.zeros(nb, dtype=np.int32)
        fw = _lib.GensysForward(_ptr(f_mat), _ptr(f_wt), _ptr(y_wt), _ptr(loose) if ne > 0 else None, _ptr(n_unst), 1)
    elif not orthonormal:
        fw = _lib.GensysForward(None, None, None, None, None, 1)
    call(fw)
    if forward:
        out = dict(f_mat=f_mat[..., 0] + 1j * f_mat[..., 1], f_wt=f_wt[..., 0] + 1j * f_wt[..., 1],
                   y_wt=y_wt[..., 0] + 1j * y_wt[..., 1], loose=loose[:, :, :ne], n_unstable=n_unst)
    if not orthonormal:
        keep = [x.copy() for x in (G1, Cc, impact, gev)]
        call(None)  # eu / status of the orthonormalised launch stay; the matrices of the launch on Pi itself come back
        for dst, src in zip((G1, Cc, impact, gev), keep):
            dst[...] = src
    gev_c = np.stack([gev[..., 0] + 1j * gev[..., 1], gev[..., 2] + 1j * gev[..., 3]], axis=-1)
    out.update(G1=G1, C=Cc, impact=impact, gev=gev_c, eu=eu, status=status, success=status == 0)
    return out


def selection_batched(B, C, D, T, A=None):
    """R = -(C T + B)^-1 D (gEconpy/solvers/shared.py:74-75); with ``A`` also the residual
    ``sum((A + B T + C T T)^2)`` (gEconpy/model/statespace.py:213)."""
    B, C, T = _check_abc(B, C, T)
    D = _f64(D, 3)
    nb, n, _ = B.shape
    k = D.shape[2]
    if D.shape[:2] != (nb, n):
        raise ValueError("D must be (batch, n, k)")
    R = np.empty((nb, n, k))
    resid = None
    if A is not None:
        A = _f64(A, 3)
        resid = np.empty(nb)
    _lib.check(
        _lib.load().dsge_selection_batched_host(_ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(T), nb, n, k, _ptr(R), _ptr(resid))
    )
    return (R, resid) if A is not None else R


def selection_adjoints_batched(B, C, T, R, R_bar):
    """Pullback of ``R = -(C T + B)^-1 D`` (gEconpy/solvers/shared.py:74-75) -> ``(B_bar, C_bar, D_bar, T_bar)``:
    ``G = -(C T + B)^-T R_bar``, ``D_bar = G``, ``B_bar = G R'``, ``C_bar = G R' T'``, ``T_bar = C' G R'``."""
    B, C, T = _check_abc(B, C, T)
    R, R_bar = _f64(R, 3), _f64(R_bar, 3)
    nb, n, _ = B.shape
    k = R.shape[2]
    if R.shape != (nb, n, k) or R_bar.shape != (nb, n, k):
        raise ValueError("R and R_bar must be (batch, n, k)")
    Bb, Cb, Tb = np.empty_like(B), np.empty_like(B), np.empty_like(B)
    Db = np.empty_like(R)
    _lib.check(_lib.load().dsge_selection_adjoints_batched_host(_ptr(B), _ptr(C), _ptr(T), _ptr(R), _ptr(R_bar), nb, n, k,
                                                                _ptr(Bb), _ptr(Cb), _ptr(Db), _ptr(Tb)))
    return Bb, Cb, Db, Tb


def policy_adjoints_batched(B, C, T, T_bar):
    """``(A_bar, B_bar, C_bar, status)``: the reverse-mode sensitivities of
    ``o1_policy_function_adjoints`` (gEconpy/solvers/shared.py:12-71) for a batch of draws."""
    B, C, T = _check_abc(B, C, T)
    T_bar = _f64(T_bar, 3)
    nb, n, _ = B.shape
    Ab, Bb, Cb = np.empty_like(B), np.empty_like(B), np.empty_like(B)
    status = np.empty(nb, dtype=np.int32)
    _lib.check(_lib.load().dsge_policy_adjoints_batched_host(_ptr(B), _ptr(C), _ptr(T), _ptr(T_bar), nb, n, _ptr(Ab),
                                                             _ptr(Bb), _ptr(Cb), _ptr(status)))
    return Ab, Bb, Cb, status


def policy_norms_batched(A, B, C, D, T, R, state_mask):
    """``deterministic_norm`` and ``stochastic_norm`` of gEconpy/model/statespace.py:1181-1204 for a
    batch of draws; ``state_mask`` is the boolean vector ``tm1_idx & t_idx`` (:1186-1193)."""
    A, B, C = _check_abc(A, B, C)
    T, R, D = _f64(T, 3), _f64(R, 3), _f64(D, 3)
    nb, n, _ = A.shape
    k = D.shape[2]
    mask = np.ascontiguousarray(np.asarray(state_mask) != 0, dtype=np.int32)
    if mask.shape != (n,):
        raise ValueError("state_mask must have one entry per variable")
    det = np.empty(nb)
    sto = np.empty(nb)
    _lib.check(_lib.load().dsge_policy_norms_batched_host(_ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(T), _ptr(R),
                                                          _ptr(mask), nb, n, k, _ptr(det), _ptr(sto)))
    return det, sto


def backward_direct_batched(A, B, D):
    """T = (-B)^-1 A, R = -B^-1 D (gEconpy/solvers/backward_looking.py:102-134)."""
    A, B = _f64(A, 3), _f64(B, 3)
    D = _f64(D, 3)
    nb, n, _ = A.shape
    k = D.shape[2]
    T = np.empty_like(A)
    R = np.empty((nb, n, k))
    _lib.check(_lib.load().dsge_backward_direct_batched_host(_ptr(A), _ptr(B), _ptr(D), nb, n, k, _ptr(T), _ptr(R)))
    return T, R


def _q_mode(Q, nb, k):
    """Infer the covariance layout from the shape (ambiguous only when batch == k)."""
    return _resolve_q(Q, None, nb, k)


def _resolve_q(Q, q_mode, nb, k):
    Q = _f64(Q)
    return Q, F.q_layout(Q.shape, q_mode, nb, k)


def lyapunov_batched(T, R, Q, q_mode=None):
    """P0 = solve_discrete_lyapunov(T, R Q R') (gEconpy/model/statespace.py:814-815) ->
    (P0, RQR, status)."""
    T, R = _f64(T, 3), _f64(R, 3)
    nb, m, _ = T.shape
    k = R.shape[2]
    Q, code = _resolve_q(Q, q_mode, nb, k)
    P0 = np.empty_like(T)
    RQR = np.empty_like(T)
    status = np.empty(nb, dtype=np.int32)
    _lib.check(_lib.load().dsge_lyapunov_batched_host(_ptr(T), _ptr(R), _ptr(Q), code, nb, m, k, _ptr(P0), _ptr(RQR), _ptr(status)))
    return P0, RQR, status


def autocorrelation_matrices_batched(T, R, Q, n_lags=10, lag_step=1, Z=None, Hdiag=None, correlation=True, q_mode=None,
                                     return_sigma=False):
    """Per-draw autocorrelation (or autocovariance) matrices at lags 0..n_lags -- the batch version of
    ``_compute_autocovariance_matrix`` (gEconpy/model/statistics/covariance.py:133-161; note that one returns lags
    0..n_lags-1) and of the graph ``sample_autocorrelation_matrices`` evaluates per posterior draw
    (gEconpy/model/statespace.py:1262-1300; ``observed=True`` <=> ``Z`` given, measurement-error variances
    ``Hdiag`` enter the lag-0 matrix).  Returns ``acf[batch, n_lags+1, dim, dim]`` (+ status [, Sigma])."""
    T, R = _f64(T, 3), _f64(R, 3)
    nb, m, _ = T.shape
    k = R.shape[2]
    Q, code = _resolve_q(Q, q_mode, nb, k)
    p = 0
    if Z is not None:
        Z = _f64(Z, 2)
        p = Z.shape[0]
        if Z.shape[1] != m:
            raise ValueError("Z must be (p, m)")
        Hdiag = None if Hdiag is None else _f64(Hdiag, 1)
    dim = p if Z is not None else m
    out = np.empty((nb, n_lags + 1, dim, dim))
    sigma = np.empty((nb, m, m)) if return_sigma else None
    status = np.empty(nb, dtype=np.int32)
    _lib.check(
        _lib.load().dsge_autocorrelation_batched_host(_ptr(T), _ptr(R), _ptr(Q), code, _ptr(Z), _ptr(Hdiag), nb, m, k, p,
                                                      int(n_lags), int(lag_step), int(bool(correlation)), _ptr(out),
                                                      _ptr(sigma), _ptr(status))
    )
    return (out, status, sigma) if return_sigma else (out, status)


def _obs_args(Z, d, Hdiag, nb, p, m):
    Z, d, Hdiag = _f64(Z), HOST.inp(d), HOST.inp(Hdiag)
    zb, db, hb = F.obs_flags(Z, d, Hdiag, nb, p, m)
    return Z, zb, d, db, Hdiag, hb


def state_hint(M):
    """Performance hint: number of columns of ``M`` (A or T, any leading batch axes) that are
    non-zero in at least one draw -- the model's state variables."""
    M = np.asarray(M)
    return int(np.count_nonzero(np.any(M != 0, axis=tuple(range(M.ndim - 1)))))


def static_hint(A, C):
    """Performance hint (``dsge_options.n_static_hint``): number of variables whose columns of ``A`` AND ``C`` are
    exactly zero in every draw -- the static variables the cycle-reduction launcher deflates."""
    A, C = np.asarray(A), np.asarray(C)
    n = A.shape[-1]
    return int(np.count_nonzero(~(np.any(A.reshape(-1, n) != 0, axis=0) | np.any(C.reshape(-1, n) != 0, axis=0))))


def selector_hint(Z):
    """Performance hint: 1 if every row of Z has exactly one non-zero entry, in distinct columns."""
    Z2 = np.asarray(Z).reshape(-1, Z.shape[-2], Z.shape[-1])
    nz = Z2 != 0
    one_per_row = np.all(nz.sum(axis=2) == 1)
    distinct = np.all(nz.sum(axis=1) <= 1)
    return int(bool(one_per_row and distinct))


def bk_eigenvalues_batched(A, B, C, tol=1e-8):
    """Batched ``compute_bk_eigenvalues`` (gEconpy/model/perturbation.py:412-445): generalized eigenvalues of the
    Sims pencil sorted by ascending modulus, plus the two counts ``check_bk_condition`` (:448-565) compares.

    Returns dict(real, imag (batch, 2n; the first ``n_eig[i]`` entries of a row are valid), n_eig, n_forward,
    n_unstable, satisfied, status)."""
    A, B, C = _check_abc(A, B, C)
    nb, n, _ = A.shape
    re = np.empty((nb, 2 * n))
    im = np.empty((nb, 2 * n))
    ne, nf, nu, st = (np.empty(nb, dtype=np.int32) for _ in range(4))
    _lib.check(
        _lib.load().dsge_bk_eigenvalues_batched_host(_ptr(A), _ptr(B), _ptr(C), nb, n, float(tol), _ptr(re), _ptr(im),
                                                     _ptr(ne), _ptr(nf), _ptr(nu), _ptr(st))
    )
    return dict(real=re, imag=im, n_eig=ne, n_forward=nf, n_unstable=nu, satisfied=(st == 0) & (nf == nu), status=st)


def kalman_logp_batched(T, R, Q, Z, y, d=None, Hdiag=None, q_mode=None, status=None,
                        jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, n_state_hint=None,
                        z_selector_hint=None, options=None, filter_type="standard"):
    """Per-draw Kalman log-likelihood (the filter DSGEStateSpace hands to PyMC,
    gEconpy/model/statespace.py:1151-1157) -> (logp, status).  ``filter_type``: see ``check_filter_type``."""
    check_filter_type(filter_type)
    T, R = _f64(T, 3), _f64(R, 3)
    y = _f64(y, 2)
    nb, m, _ = T.shape
    if m > _lib.MAX_N:
        # More than 64 variables: the filter of the model restricted to F = {variables with a non-zero column of T in some
        # draw} u {observed variables} is the same filter (x_t[F] depends on x_{t-1}[F] only, y_t on x_t[F] only), and the
        # device kernels take |F| <= 64 -- the gather the fused entry point does on the device (csrc/dsge_big.hpp), here on
        # the host because T and R arrive as host arrays.  Exact zeros only: a T whose non-state columns carry rounding noise
        # keeps them, and the call fails loudly instead of dropping them.
        Zf = _f64(Z)
        # (a draw that arrives with a non-zero status is skipped by the filter anyway, and a failed solve may have left NaN in
        #  its T -- NaN compares non-zero --: neither may widen F for the whole batch)
        live = np.ones(nb, dtype=bool) if status is None else (np.asarray(status).reshape(-1) == 0)
        Tl = T[live]
        keep = np.any(np.isfinite(Tl) & (Tl != 0.0), axis=(0, 1)) | np.any(Zf.reshape(-1, m) != 0.0, axis=0)
        idx = np.flatnonzero(keep)
        if idx.size > _lib.MAX_N:
            raise _lib.DsgeTooLargeError(f"kalman_logp_batched: {idx.size} state and observed variables, the filter kernels "
                                         f"take at most {_lib.MAX_N}")
        T = np.ascontiguousarray(T[:, idx][:, :, idx])
        R = np.ascontiguousarray(R[:, idx])
        Z = np.ascontiguousarray(Zf[..., idx])
        m = idx.size
        n_state_hint = None
    k = R.shape[2]
    T_len, p = y.shape
    Q, code = _resolve_q(Q, q_mode, nb, k)
    Z, zb, d, db, Hdiag, hb = _obs_args(Z, d, Hdiag, nb, p, m)
    st = np.zeros(nb, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32).copy()
    logp = np.empty(nb)
    ns = state_hint(T) if n_state_hint is None else int(n_state_hint)
    zs = selector_hint(Z) if z_selector_hint is None else int(z_selector_hint)
    with _lib.options_scope(options):
        _lib.check(
            _lib.load().dsge_kalman_logp_batched_host(
                _ptr(T), _ptr(R), _ptr(Q), code, _ptr(Z), zb, _ptr(d), db, _ptr(Hdiag), hb, _ptr(y), nb, m, k, p, T_len,
                float(jitter), float(missing_fill_value), ns, zs, _ptr(logp), _ptr(st)
            )
        )
    return logp, st


def kalman_filter_outputs_batched(T, R, Q, Z, y, d=None, Hdiag=None, q_mode=None, status=None, jitter=JITTER_DEFAULT,
                                 missing_fill_value=MISSING_FILL, full_covariances=False, options=None):
    """Per-step filter outputs for a batch of draws -- what ``save_kalman_filter_outputs_in_idata=True`` stores
    (gEconpy/model/statespace.py:1145, 1151-1157): dict(ll (batch, T_len), predicted_states / filtered_states (batch, T_len, m),
    predicted_covs / filtered_covs: the diagonals (batch, T_len, m), or the matrices (batch, T_len, m, m) with
    ``full_covariances``, status).  ``ll.sum(axis=1)`` is the log-likelihood of ``kalman_logp_batched``."""
    T, R = _f64(T, 3), _f64(R, 3)
    y = _f64(y, 2)
    nb, m, _ = T.shape
    k = R.shape[2]
    T_len, p = y.shape
    Q, code = _resolve_q(Q, q_mode, nb, k)
    Z, zb, d, db, Hdiag, hb = _obs_args(Z, d, Hdiag, nb, p, m)
    st = np.zeros(nb, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32).copy()
    cshape = (nb, T_len, m, m) if full_covariances else (nb, T_len, m)
    out = dict(ll=np.empty((nb, T_len)), predicted_states=np.empty((nb, T_len, m)), filtered_states=np.empty((nb, T_len, m)),
               predicted_covs=np.empty(cshape), filtered_covs=np.empty(cshape))
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        _lib.check(
            _lib.load().dsge_kalman_filter_outputs_batched_host(
                _ptr(T), _ptr(R), _ptr(Q), code, _ptr(Z), zb, _ptr(d), db, _ptr(Hdiag), hb, _ptr(y), nb, m, k, p, T_len, float(jitter),
                float(missing_fill_value), _ptr(out["ll"]), _ptr(out["predicted_states"]), _ptr(out["filtered_states"]),
                _ptr(out["predicted_covs"]), _ptr(out["filtered_covs"]), int(bool(full_covariances)), _ptr(st)
            )
        )
    out["status"] = st
    return out


def kalman_logp_segments_batched(T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None, jitter=JITTER_DEFAULT,
                                 missing_fill_value=MISSING_FILL, options=None, outputs=F.SEGMENT_OUTPUTS, q_mode=None, status=None):
    """Kalman log-likelihood across DATED STRUCTURAL BREAKS per draw (include/dsge_hip.h, ``dsge_kalman_logp_segments_batched``;
    docs/design/segmented_filter.md): the system matrices are piecewise constant in time, segment s from period ``seg_start[s]``
    on (``seg_start[0] == 0``, strictly increasing, shared by all draws, at most ``_lib.MAX_SEGMENTS`` entries).  ``T``
    (batch, S, m, m), ``R`` (batch, S, m, k); ``q`` (S, k), (batch, S, k), (S, k, k) or (batch, S, k, k); ``Z`` (S, p, m) or
    (batch, S, p, m); ``d``, ``Hdiag``: None, (S, p) or (batch, S, p); ``a0`` (batch, m): the predicted mean of period 0 (None: 0);
    ``P0`` (batch, m, m): its covariance (None: the stationary covariance of segment 0); ``shift`` (batch, S, m): added to the
    filtered mean once, at the boundary into segment s, before the product with ``T_s`` (row 0 is never read).  ``outputs``: which
    of logp, ll, a_last, P_last are computed.  Returns dict(logp (batch,), ll (batch, T_len), a_last (batch, m), P_last
    (batch, m, m): the FILTERED moments of the last period, what ``forecast_batched`` takes as ``a0``, ``P0``; status)."""
    return F.kalman_logp_segments(HOST, "kalman_logp_segments_batched", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d, a0=a0, P0=P0,
                                  shift=shift, q_mode=q_mode, status=status, jitter=jitter, missing_fill=missing_fill_value,
                                  options=options, outputs=outputs)


def solve_kalman_logp_segments_batched(A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                       solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                       missing_fill_value=MISSING_FILL, options=None, outputs=F.SEGMENT_OUTPUTS, q_mode=None,
                                       n_lead_hint=0):
    """``A .. D`` (batch, S, n, n | k) -> ``T``, ``R`` of every (draw, segment) by the solver entry ``solver`` names
    ("cycle_reduction", "gensys", "backward_direct") on the flattened batch, then ``kalman_logp_segments_batched``.  A draw whose
    solve fails in any segment gets ``logp = -inf`` and the OR of the segments' status bits.  Returns the filter's dict plus
    ``T`` (batch, S, n, n) and ``R`` (batch, S, n, k)."""
    return F.solve_kalman_logp_segments(HOST, "solve_kalman_logp_segments_batched", A, B, C, D, q, Z, y, seg_start, solver=solver,
                                        tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options, Hdiag=Hdiag, d=d, a0=a0,
                                        P0=P0, shift=shift, q_mode=q_mode, jitter=jitter, missing_fill=missing_fill_value,
                                        outputs=outputs)


segment_gradient_scratch_bytes_per_draw = F.segment_gradient_scratch_bytes_per_draw


def kalman_logp_segments_grad_batched(T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None, jitter=JITTER_DEFAULT,
                                      missing_fill_value=MISSING_FILL, scratch_limit_bytes=None, options=None,
                                      outputs=F.SEGMENT_GRADIENT_OUTPUTS, q_mode=None, status=None, out=None):
    """``logp`` of ``kalman_logp_segments_batched`` (same arguments, same layouts, the same bits) and its GRADIENT with respect to
    every entry of every input, by a hand-written reverse sweep on the device (include/dsge_hip.h,
    ``dsge_kalman_logp_segments_grad_batched``; docs/design/segmented_gradient.md).  ``outputs``: which of T_bar (batch, S, m, m),
    R_bar (batch, S, m, k), q_bar (batch, S, k) -- returned as Q_bar (batch, S, k, k), the symmetric convention, for a full
    covariance --, Z_bar (batch, S, p, m), d_bar, h_bar (batch, S, p), shift_bar (batch, S, m; row 0 zero), a0_bar (batch, m),
    P0_bar (batch, m, m; zero unless ``P0`` is given) are computed; any subset has the bits of the full call.  Cotangents are per
    draw also for shared inputs (sum over the batch).  A failed draw gets ``logp = -inf`` and zeros.  ``scratch_limit_bytes``
    (default 2 GiB) counts ``segment_gradient_scratch_bytes_per_draw`` per draw.  Returns a dict of logp, the cotangents (None
    where not asked for) and status."""
    return F.kalman_logp_segments_grad(HOST, "kalman_logp_segments_grad_batched", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d, a0=a0,
                                       P0=P0, shift=shift, q_mode=q_mode, status=status, jitter=jitter,
                                       missing_fill=missing_fill_value, scratch_limit_bytes=scratch_limit_bytes, options=options,
                                       outputs=outputs, out=out)


def solve_kalman_logp_segments_grad_batched(A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                            solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                            missing_fill_value=MISSING_FILL, scratch_limit_bytes=None, options=None,
                                            outputs=F.SEGMENT_GRADIENT_OUTPUTS, q_mode=None, n_lead_hint=0, out=None):
    """``A .. D`` (batch, S, n, n | k), n <= 56, solved per (draw, segment) as ``solve_kalman_logp_segments_batched`` solves them
    (``solver``: "cycle_reduction" or "gensys"; "backward_direct" has no adjoint and is refused), ``kalman_logp_segments_grad_batched``,
    then the pullbacks through R and the policy function on the flattened batch.  Returns that dict plus A_bar, B_bar, C_bar
    (batch, S, n, n), D_bar (batch, S, n, k), T and R.  A draw whose solve or adjoint fails in any segment gets ``-inf``, the OR of
    the status bits and zero cotangents."""
    return F.solve_kalman_logp_segments_grad(HOST, "solve_kalman_logp_segments_grad_batched", A, B, C, D, q, Z, y, seg_start,
                                             solver=solver, tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options,
                                             Hdiag=Hdiag, d=d, a0=a0, P0=P0, shift=shift, q_mode=q_mode, jitter=jitter,
                                             missing_fill=missing_fill_value, scratch_limit_bytes=scratch_limit_bytes,
                                             outputs=outputs, out=out)


def smoother_scratch_bytes_per_draw(m, T_len):
    """Bytes of library scratch the smoother's forward pass stores per draw (what ``scratch_limit_bytes`` counts):
    ``2 T_len m^2 + 2 T_len m`` doubles."""
    return 8 * (2 * T_len * m * m + 2 * T_len * m)


def kalman_smoother_batched(T, R, Q, Z, y, d=None, Hdiag=None, q_mode=None, status=None, jitter=JITTER_DEFAULT,
                            missing_fill_value=MISSING_FILL, full_covariances=False, rank_tol=None, scratch_limit_bytes=None,
                            options=None):
    """Smoothed states, covariances and structural shocks for a batch of draws -- the "smoothed" output of
    ``save_kalman_filter_outputs_in_idata=True`` (gEconpy/model/statespace.py:1145, 1151-1157; gEconpy/plotting.py:1791-1835):
    the fixed-interval (Rauch-Tung-Striebel) recursion on the outputs of ``kalman_filter_outputs_batched`` with the
    pseudo-inverse of the predicted covariance (include/dsge_hip.h, ``dsge_kalman_smoother_batched``).  Returns dict(ll (batch,
    T_len), smoothed_states (batch, T_len, m), smoothed_covs: diagonals (batch, T_len, m) or, with ``full_covariances``,
    (batch, T_len, m, m), smoothed_shocks (batch, T_len, k) with ``[:, 0] = NaN`` by definition, status).  ``options`` carries
    the filter conventions (``_lib.filter_conventions``); ``rank_tol`` (default 1e-10) sets the rank of the range basis;
    ``scratch_limit_bytes`` (default 2 GiB) bounds the stored forward pass (``smoother_scratch_bytes_per_draw`` per draw)."""
    return F.kalman_smoother(HOST, "kalman_smoother_batched", T, R, Q, Z, y, d=d, Hdiag=Hdiag, q_mode=q_mode, status=status,
                             jitter=jitter, missing_fill=missing_fill_value, cov=True, full=full_covariances, rank_tol=rank_tol,
                             scratch_limit_bytes=scratch_limit_bytes, options=options)


segment_smoother_scratch_bytes_per_draw = F.segment_smoother_scratch_bytes_per_draw


def kalman_smoother_segments_batched(T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None, jitter=JITTER_DEFAULT,
                                     missing_fill_value=MISSING_FILL, full_covariances=False, rank_tol=None, scratch_limit_bytes=None,
                                     options=None, outputs=F.SEGMENT_SMOOTHER_OUTPUTS, q_mode=None, status=None):
    """Smoothed states, covariances and structural shocks ACROSS DATED STRUCTURAL BREAKS per draw, with the per-step filter outputs
    they stand on (include/dsge_hip.h, ``dsge_kalman_smoother_segments_batched``; docs/design/segmented_smoother.md): the
    counterpart of ``kalman_smoother_batched`` for the inputs of ``kalman_logp_segments_batched`` (same arguments, same layouts).
    Step t of the backward pass uses the matrices of the segment of period t + 1; ``smoothed_states[:, t]`` is in the coordinates of
    the segment of period t, ``smoothed_shocks[:, 0]`` is NaN by definition.  ``outputs``: which of ll (batch, T_len), a_pred, a_filt
    (batch, T_len, m), P_pred, P_filt, smoothed_covs (diagonals (batch, T_len, m) or, with ``full_covariances``, (batch, T_len, m,
    m)), smoothed_states (batch, T_len, m), smoothed_shocks (batch, T_len, k) are computed -- without smoothed_covs the covariance
    recursion is skipped.  ``scratch_limit_bytes`` (default 2 GiB) counts ``segment_smoother_scratch_bytes_per_draw`` per draw.
    Returns a dict of the outputs (None where not asked for) and status."""
    return F.kalman_smoother_segments(HOST, "kalman_smoother_segments_batched", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d, a0=a0,
                                      P0=P0, shift=shift, q_mode=q_mode, status=status, jitter=jitter,
                                      missing_fill=missing_fill_value, full=full_covariances, rank_tol=rank_tol,
                                      scratch_limit_bytes=scratch_limit_bytes, options=options, outputs=outputs)


def solve_kalman_smoother_segments_batched(A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                           solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                           missing_fill_value=MISSING_FILL, full_covariances=False, rank_tol=None,
                                           scratch_limit_bytes=None, options=None, outputs=F.SEGMENT_SMOOTHER_OUTPUTS, q_mode=None,
                                           n_lead_hint=0):
    """``A .. D`` (batch, S, n, n | k) -> ``T``, ``R`` of every (draw, segment) as ``solve_kalman_logp_segments_batched`` solves
    them, then ``kalman_smoother_segments_batched``.  A draw whose solve fails in any segment has NaN in every output and the OR of
    the segments' status bits.  Returns the smoother's dict plus ``T`` and ``R``."""
    return F.solve_kalman_smoother_segments(HOST, "solve_kalman_smoother_segments_batched", A, B, C, D, q, Z, y, seg_start,
                                            solver=solver, tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options,
                                            Hdiag=Hdiag, d=d, a0=a0, P0=P0, shift=shift, q_mode=q_mode, jitter=jitter,
                                            missing_fill=missing_fill_value, full=full_covariances, rank_tol=rank_tol,
                                            scratch_limit_bytes=scratch_limit_bytes, outputs=outputs)


simulation_smoother_scratch_bytes_per_draw = F.simulation_smoother_scratch_bytes_per_draw


def stationary_factor(T, R, Q, q_mode=None):
    """F (batch, m, m) with ``F F' = P0 = solve_discrete_lyapunov(T, R Q R')`` per draw: ``x0 = z F'`` with standard normal z
    is a draw of the pre-sample state.  P0 from ``dsge_lyapunov_batched``, ``F = V sqrt(max(lambda, 0))`` from
    ``numpy.linalg.eigh`` (P0 is singular for every DSGE model, so no Cholesky factor)."""
    return F.stationary_factor(HOST, "stationary_factor", T, R, Q, q_mode=q_mode)


def simulation_smoother_batched(T, R, Q, Z, y, n_paths=1, d=None, Hdiag=None, q_mode=None, x0=None, eps=None, eta=None, rng=None,
                                return_draws=False, status=None, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL,
                                rank_tol=None, scratch_limit_bytes=None, options=None):
    """``n_paths`` JOINT posterior draws of the whole state path and of the structural shocks per parameter draw, conditional
    on the data -- what ``sample_conditional_posterior`` of the pymc_extras model behind ``DSGEStateSpace`` is used for (its
    draws are per-step marginals, these are joint over time) and what Dynare's simulation smoother draws: Durbin and Koopman's
    mean correction on ``kalman_smoother_batched`` (include/dsge_hip.h, ``dsge_simulation_smoother_batched``).  The draws the
    correction starts from -- ``x0`` (n_paths, m) ~ N(0, P0), ``eps`` (n_paths, T_len, k) ~ N(0, Q), ``eta``
    (n_paths, T_len, p) ~ N(0, diag Hdiag), each shared by all draws or with a leading batch axis -- are the caller's, or, where
    None, made here from standard normals of ``rng`` (a seed or ``np.random.Generator``): ``eps = z sqrt(q)`` / ``z S'`` with the
    symmetric-eigen factor ``S S' = Q``, ``eta = z sqrt(H)`` (none without ``Hdiag``), ``x0 = z F'`` with ``stationary_factor``.
    All-zero draws give the smoothed means (pass zero arrays: a None is drawn).  Returns dict(states (batch, n_paths, T_len, m), shocks (batch, n_paths, T_len, k)
    with ``[:, :, 0] = NaN`` by the smoother's definition, ll (batch, T_len), status[, x0, eps, eta with ``return_draws``]).
    ``scratch_limit_bytes`` counts ``simulation_smoother_scratch_bytes_per_draw(m, T_len, n_paths)`` per draw."""
    return F.simulation_smoother(HOST, "simulation_smoother_batched", T, R, Q, Z, y, n_paths=n_paths, d=d, Hdiag=Hdiag, q_mode=q_mode,
                                 x0=x0, eps=eps, eta=eta, rng=rng, return_draws=return_draws, status=status, jitter=jitter,
                                 missing_fill=missing_fill_value, rank_tol=rank_tol, scratch_limit_bytes=scratch_limit_bytes,
                                 options=options)


def simulate_batched(T, R, eps, n_steps=None, x0=None, status=None):
    """Simulated paths ``x[b, s, t] = T_b x[b, s, t-1] + R_b eps[b, s, t]`` for a batch of draws -- the loop of
    ``_simulate_linear_system`` (gEconpy/model/simulate.py:171-182) that ``simulate`` (:320-430) runs once per trajectory, for
    every draw and path at once (include/dsge_hip.h, ``dsge_simulate_batched``).  ``eps``: (n_paths, n_shock_steps, k) shared by
    all draws or (batch, n_paths, n_shock_steps, k) -- the caller draws the shocks, as ``simulate`` does from its
    ``random_seed``; ``n_steps`` (default n_shock_steps) may exceed n_shock_steps: the later steps have no shock.  ``x0``:
    (n_paths, m) or (batch, n_paths, m), default zero (the reference's start).  ``status``: optional (batch,) int32, a draw
    with a non-zero word gets NaN.  Returns dict(paths (batch, n_paths, n_steps, m))."""
    return dict(paths=F.simulate(HOST, "simulate_batched", T, R, eps, n_steps=n_steps, x0=x0, status=status))


def shock_decomposition_batched(T, R, states, shocks, groups=None, variables=None, Z=None, remainder=True, status=None):
    """Historical shock decomposition for a batch of draws: how much of every variable's smoothed path each structural shock
    explains (include/dsge_hip.h, ``dsge_shock_decomposition_batched``).  From the smoother:
    ``s = kalman_smoother_batched(T, R, Q, Z, y)`` -> ``shock_decomposition_batched(T, R, s["smoothed_states"],
    s["smoothed_shocks"])``; from the simulation smoother: ``s = simulation_smoother_batched(T, R, Q, Z, y, n_paths=...)`` ->
    ``shock_decomposition_batched(T, R, s["states"], s["shocks"])``.  ``states`` / ``shocks``: (batch, T_len, m) / (batch, T_len, k)
    or (batch, n_paths, T_len, .); period 0 of ``shocks`` (NaN by the smoother's definition) is never read: period 0 is the initial
    condition alone.  ``groups``: a sequence of sequences of shock indices that partitions 0 .. k-1 (default: every shock its
    own group; at most 15 groups, so a model with more shocks groups them).  ``variables``: the variables wanted, distinct, any
    order (default all; ``()`` with ``Z``: the observed decomposition alone).  ``Z``: (p, m) or (batch, p, m), adds the decomposition
    of ``Z x`` (the intercept d is not a component).  ``remainder``: append ``x - (sum of the other components)`` -- what the filter
    conventions leave between the smoothed path and the exact path of the smoothed shocks (1e-5 of max|x| by default, rounding
    with ``jitter_on_P=False``), so that the components add up to ``x``.  ``status``: optional (batch,) int32, a draw with a
    non-zero word gets NaN.  Returns dict(contributions (..., n_variables, C) or None, observed (..., p, C) or None, components:
    the names of the last axis -- the group indices, ``"initial"``[, ``"remainder"``])."""
    return F.shock_decomposition(HOST, "shock_decomposition_batched", T, R, states, shocks, groups=groups, variables=variables, Z=Z,
                                 remainder=remainder, status=status)


def conditional_forecast_batched(T, R, Q, x0, conditions, n_steps, Z=None, d=None, eps=None, n_paths=None, free_shocks=None,
                                 q_mode=None, status=None, rank_tol=0.0):
    """Conditional forecasts for a batch of draws: paths ``x[t] = T x[t-1] + R e[t]``, ``t = 0 .. n_steps-1``, from the known state
    ``x[-1] = x0`` that are forced through given future values of some observables ``d + Z x`` -- the hard conditions of Waggoner
    and Zha (1999); include/dsge_hip.h, ``dsge_conditional_forecast_batched``.  ``conditions``: (h_c, p), (batch, h_c, p) or
    (batch, n_paths, h_c, p) with NaN = free (the NaN pattern must be the same for all draws and paths, else ``ValueError``), or the
    triple ``(cond_t, cond_j, values)``.  ``x0``: (m,), (batch, m) or (batch | 1, n_paths | 1, m).  ``eps``: the baseline shocks,
    (n_paths, n_shock_steps, k) or (batch, n_paths, n_shock_steps, k), None = zeros.  ``free_shocks``: the indices (or a boolean
    mask) of the shocks that may move, default all; the others keep their baseline values bit for bit.  The free shocks of the
    periods up to the last conditioned one get the correction of minimum ``Q_FF^-1`` norm that meets the conditions:
    (1) with all shocks free and ``eps ~ N(0, Q)`` the paths are exact draws from the distribution conditional on the scenario, and
    with ``eps=None`` the path is its mean (the smoothed mean of a Kalman filter + smoother from the known ``x0`` with the
    conditions as noiseless observations); (2) with as many conditioned series in EVERY period up to the last conditioned one as
    there are free shocks the system is square and the answer does not depend on ``Q`` -- the controlled-shock conditional forecast
    of Dynare; (3) with a full ``Q`` and a proper subset of free shocks the norm uses the block ``Q_FF`` and no distribution is
    claimed.  A draw whose conditions cannot be met (a Cholesky pivot of ``G <= rank_tol max diag G``, default 1e-10) gets
    ``ST_COND_SINGULAR`` (512) in ``status`` and NaN everywhere; so does a draw with a non-zero incoming ``status``.
    Returns dict(x (batch, n_paths, n_steps, m), shocks (.., k): the shocks that generate ``x``, observed (.., p), status)."""
    return F.conditional_forecast(HOST, "conditional_forecast_batched", T, R, Q, x0, conditions, n_steps, Z=Z, d=d, eps=eps,
                                  n_paths=n_paths, free_shocks=free_shocks, q_mode=q_mode, status=status, rank_tol=rank_tol)


expected_shocks_from_news = F.expected_shocks_from_news


def anticipated_paths_batched(B, C, T, R, eps, n_steps=None, mode="perfect_foresight", x0=None, Z=None, d=None, status=None,
                              rank_tol=0.0, outputs=("x",)):
    """Paths with ANTICIPATED shocks for a batch of draws -- forward guidance, a pre-announced fiscal path, news shocks; the
    linearised counterpart of the reference's stacked-time perfect-foresight solver (gEconpy/model/perfect_foresight/);
    include/dsge_hip.h, ``dsge_anticipated_paths_batched``.  The model is ``A x[t-1] + B x[t] + C E_t x[t+1] + D eps[t] = 0`` with
    the solution ``T`` and ``R = -(B + C T)^-1 D`` as the solver entries return them; with ``G = -(B + C T)^-1 C``:
    ``x[t] = T x[t-1] + w[t]``, ``w[t] = sum_j G^j R E_t eps[t+j]``, ``x[-1] = x0``, ``t = 0 .. n_steps-1``.
    ``mode="perfect_foresight"``: ``eps`` (n_paths, n_shock_steps, k) or (batch, n_paths, n_shock_steps, k) is the whole shock
    path, known at ``t = 0``; ``n_shock_steps`` may exceed ``n_steps`` (default n_shock_steps).  ``mode="news"``: ``eps``
    (n_paths, n_shock_steps, n_lead + 1, k) or with a leading batch axis holds the expected shocks ``e[t][j] = E_t eps[t+j]``
    (``expected_shocks_from_news`` makes them from arrivals); ``n_steps >= n_shock_steps``; ``n_lead = 0`` is ``simulate_batched``.
    ``x0``: (n,), (n_paths, n) or (batch | 1, n_paths | 1, n), default zero.  ``Z`` (p, n) or (batch, p, n) and ``d`` (p,) or
    (batch, p): the observation equation of the output ``"observed"``.  ``outputs``: any of ``"x"``, ``"w"`` (the anticipation
    term ``x[t] - T x[t-1]``), ``"observed"``, ``"G"``.  A draw whose ``B + C T`` is singular (a pivot ``<= rank_tol max|M|``,
    default 1e-14) gets ``ST_ANTICIPATION_SINGULAR`` (2048) in ``status`` and NaN everywhere; so does a draw with a non-zero
    incoming ``status``.  At most 64 variables.  Returns dict(x, w (batch, n_paths, n_steps, n), observed (.., p), G (batch, n, n)
    -- those requested -- and status)."""
    return F.anticipated_paths(HOST, "anticipated_paths_batched", B, C, T, R, eps, n_steps=n_steps, mode=mode, x0=x0, Z=Z, d=d,
                               status=status, rank_tol=rank_tol, outputs=outputs)


def constrained_paths_batched(B, C, T, R, eps, c, bound, shock, horizon, n_steps=None, x0=None, Z=None, d=None, status=None,
                              rank_tol=0.0, max_iter=0, outputs=("x",)):
    """Perfect-foresight paths under an OCCASIONALLY BINDING BOUND for a batch of draws -- the zero lower bound on a policy rate;
    include/dsge_hip.h, ``dsge_constrained_paths_batched``.  The model, ``eps`` (n_paths, n_shock_steps, k) or (batch, n_paths,
    n_shock_steps, k), ``x0``, ``Z``, ``d`` and ``status`` are those of ``anticipated_paths_batched`` in mode "perfect_foresight".
    ``c'x[t] >= bound`` is enforced in the periods ``t < horizon`` (1 .. 64, at most ``n_steps``) by anticipated shadow shocks
    ``nu[t] >= 0`` on shock column ``shock``: ``w[t] = G w[t+1] + R (eps[t] + nu[t] e_shock)``, ``gap[t] = c'x[t] - bound``,
    ``nu[h] gap[h] = 0``; the regime iteration of the header solves for them (at most ``max_iter`` solves, default 64).
    ``c``: (n,) or (batch, n); ``bound``: a number or (batch,).  ``outputs``: any of ``"x"``, ``"w"``, ``"observed"``, ``"nu"``
    (batch, n_paths, horizon), ``"gap"`` (batch, n_paths, n_steps), ``"Mz"`` (batch, horizon, horizon), ``"path_status"`` and
    ``"iters"`` (batch, n_paths) int32.  ``path_status`` bits: ``OBC_NO_REGIME`` (1), ``OBC_SINGULAR`` (2) -- NaN in the path, and
    ``ST_CONSTRAINT_UNRESOLVED`` (4096) in the draw's ``status`` --, ``OBC_BEYOND_HORIZON`` (4: the bound is violated at some
    ``t >= horizon``; the path is returned), ``OBC_SKIPPED`` (8: the draw came in failed or ``B + C T`` is singular).  Returns
    dict(those requested, status)."""
    return F.constrained_paths(HOST, "constrained_paths_batched", B, C, T, R, eps, c, bound, shock, horizon, n_steps=n_steps, x0=x0, Z=Z,
                               d=d, status=status, rank_tol=rank_tol, max_iter=max_iter, outputs=outputs)


def constrained_simulate_batched(B, C, T, R, eps, c, bound, shock, horizon, n_steps=None, x0=None, Z=None, d=None, status=None,
                                 rank_tol=0.0, max_iter=0, outputs=("x",)):
    """STOCHASTIC SIMULATION at an occasionally binding bound for a batch of draws; include/dsge_hip.h,
    ``dsge_constrained_simulate_batched``.  The model, ``c``, ``bound``, ``shock``, ``horizon`` (1 .. 64, no relation to ``n_steps``),
    ``x0``, ``Z``, ``d``, ``status``, ``rank_tol`` and ``max_iter`` are those of ``constrained_paths_batched``, but ``eps``
    (n_paths, n_shock_steps, k) or (batch, n_paths, n_shock_steps, k) holds SURPRISE shocks: ``eps[t]`` arrives at ``t``, agents
    re-plan, and the linear complementarity problem is solved again every period.  With ``xu = T x[t-1] + R eps[t]``:
    ``q[h] = c'T^h xu - bound``, the plan ``nu >= 0`` of the regime iteration on ``(Mz, q)``, ``x[t] = xu + W nu``,
    ``W[:, j] = G^j R[:, shock]``.  ``n_steps`` defaults to the shock steps and may not be below them (zero shocks afterwards).
    ``outputs``: any of ``"x"``, ``"observed"``, ``"gap"`` (``c'x[t] - bound``), ``"shadow"`` (``nu[0]`` of the plan of ``t``, the
    shadow shock realised) (batch, n_paths, n_steps[, n | p]), ``"plan"`` (batch, n_paths, n_steps, horizon), ``"duration"`` (the
    periods the bound is expected to bind in the plan of ``t``) and ``"iters"`` (batch, n_paths, n_steps) int32, ``"Mz"`` (batch,
    horizon, horizon), ``"path_status"`` and ``"fail_step"`` (batch, n_paths) int32.  ``path_status`` bits: ``OBC_NO_REGIME`` (1),
    ``OBC_SINGULAR`` (2) -- the path keeps the periods before ``fail_step`` and has NaN from it on, and its draw gets
    ``ST_CONSTRAINT_UNRESOLVED`` (4096) --, ``OBC_SKIPPED`` (8), ``OBC_HORIZON_SHORT`` (16: in some period the last period of the
    plan binds; the path is returned).  Returns dict(those requested, status)."""
    return F.constrained_simulate(HOST, "constrained_simulate_batched", B, C, T, R, eps, c, bound, shock, horizon, n_steps=n_steps, x0=x0,
                                  Z=Z, d=d, status=status, rank_tol=rank_tol, max_iter=max_iter, outputs=outputs)


hp_gain, bandpass_gain = F.hp_gain, F.bandpass_gain


def spectral_moments_batched(T, R, Q, n_grid=512, n_lags=10, Z=None, Hdiag=None, gain=None, correlation=False, spectrum=False,
                             q_mode=None, status=None, rank_tol=None, scratch_limit_bytes=None, acov=True):
    """Spectral densities and the exact autocovariances of linearly filtered series for a batch of draws -- the frequency-domain
    route of Dynare's ``hp_filter`` theoretical moments; include/dsge_hip.h, ``dsge_spectral_moments_batched``.  The series are
    ``w = Z x`` (``Z`` (p, m) or (batch, p, m); None: the states themselves) of ``x_t = T x_{t-1} + R e_t``, ``e ~ (0, Q)``, plus
    white noise ``Hdiag``.  On the grid ``w_n = 2 pi n / n_grid``, ``n = 0 .. n_grid / 2``: ``F_n = H_n Q H_n^H (+ diag(Hdiag))``,
    ``H_n = Z (I - exp(-i w_n) T)^-1 R``; ``spectrum[b, n] = F_n / 2 pi`` (unfiltered) and
    ``acov[b, j] = (1 / N) sum_n c_n gain_n Re(F_n exp(i w_n j)) = E[w_t w_{t-j}']`` of the filtered series, ``j = 0 .. n_lags``.
    ``gain`` (n_grid / 2 + 1,): the squared gain of the filter (``hp_gain``, ``bandpass_gain``, or any), None = ones.  ``n_grid`` is
    part of the definition: the unfiltered autocovariances are folded modulo ``n_grid``.  ``correlation``: every lag divided by
    ``std std'``.  A draw with a root of ``T`` on the unit circle at a solved grid frequency gets ``ST_SPECTRAL_SINGULAR`` (1024)
    in ``status`` and NaN; frequencies of zero gain are not solved unless ``spectrum`` is wanted, so HP-filtered moments of a
    unit-root model are finite.  ``rho(T) > 1`` is not detected: pass the solver's ``status``.  ``acov=False``: the spectrum only.
    Returns dict(acov (batch, n_lags + 1, dim, dim), [spectrum complex128 (batch, nf, dim, dim)], freqs (nf,), status)."""
    return F.spectral_moments(HOST, "spectral_moments_batched", T, R, Q, n_grid=n_grid, n_lags=n_lags, Z=Z, Hdiag=Hdiag, gain=gain,
                              correlation=correlation, spectrum=spectrum, acov=acov, q_mode=q_mode, status=status,
                              rank_tol=rank_tol, scratch_limit_bytes=scratch_limit_bytes)


def impulse_response_batched(T, R, n_steps=40, S=None, weights=None, fevd=False, irf=True, status=None):
    """Impulse responses ``irf[b, j, h] = T_b^h R_b S[:, j]`` for a batch of draws -- ``impulse_response_function``
    (gEconpy/model/simulate.py:201-317; its loop over shocks :300-311 calls ``_simulate_linear_system`` :171-182 once per
    shock) for every draw and impulse at once (include/dsge_hip.h, ``dsge_irf_batched``).  ``S``: (k, c) or (batch, k, c),
    impulse j is its column j; default ``I_k`` (unit impulses to every shock).  The reference's modes: ``shock_size`` ->
    ``S = diag(s)``; ``return_individual_shocks=False`` -> ``S = s[:, None]``; orthogonalised ``shock_cov`` ->
    ``S = cholesky(Q)``.  ``fevd=True`` adds the forecast-error variance decomposition with respect to these impulses
    (``weights``: (c,) or (batch, c), default ones; an extension, the reference has none); ``irf=False`` skips the responses.
    Returns dict(irf (batch, c, n_steps, m) or None, fevd (batch, n_steps, m, c) or None)."""
    return F.impulse_response(HOST, "impulse_response_batched", T, R, n_steps=n_steps, S=S, weights=weights, fevd=fevd, irf=irf,
                              status=status)


def forecast_batched(T, R, Q, a0, P0=None, n_steps=10, Z=None, d=None, Hdiag=None, q_mode=None, covariances="diag",
                     status=None):
    """Out-of-sample forecast moments for a batch of draws -- the ``forecast`` of the pymc_extras state-space model that
    ``DSGEStateSpace`` extends (gEconpy/model/statespace.py:51), which iterates ``x = T x + R eps`` from the last filtered
    state per draw: ``a_h = T a_{h-1}``, ``P_h = sym(T P_{h-1} T') + sym(R Q R')``, ``y_h = Z a_h + d``,
    ``F_h = sym(Z P_h Z') + diag(H)`` for h = 1..n_steps (include/dsge_hip.h, ``dsge_forecast_batched``).  ``a0``: (batch, m);
    ``P0``: (batch, m, m) or None for zero; ``covariances``: ``"diag"``, ``"full"`` or ``None`` (the covariance recursion is
    skipped).  With ``Z`` ((p, m) or (batch, p, m)) the observation moments are returned too.  Recipe from the filter:
    ``kalman_filter_outputs_batched(..., full_covariances=True)`` -> ``a0 = filtered_states[:, -1]``,
    ``P0 = filtered_covs[:, -1]``.  Returns dict(states (batch, n_steps, m), covs, observed (batch, n_steps, p) or None,
    observed_covs (batch, n_steps, p, p) or None)."""
    return F.forecast(HOST, "forecast_batched", T, R, Q, a0, P0=P0, n_steps=n_steps, Z=Z, d=d, Hdiag=Hdiag, q_mode=q_mode,
                      covariances=covariances, status=status)


def solve_kalman_logp_batched(A, B, C, D, Q, Z, y, d=None, Hdiag=None, q_mode=None, solver="cycle_reduction",
                              tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL,
                              return_policy=False, n_state_hint=None, z_selector_hint=None, n_lead_hint=None,
                              options=None, add_solver_success_check=True, filter_type="standard"):
    """One fused evaluation per draw: A,B,C,D -> T,R -> P0 -> logp.  ``tol``/``max_iter``
    default to what ``DSGEStateSpace.configure`` passes (statespace.py:835-836).
    ``filter_type`` (build.py:577): only "standard" is built, the others raise (``check_filter_type``).
    ``add_solver_success_check=False`` (the reference's default, statespace.py:1148): a draw whose cycle reduction fails carries
    ``T = 0`` on and gets the finite log-likelihood of that system (``DSGE_SOLVER_FLAG_ZERO_T_ON_FAILURE``); the default here
    is the safe one, ``-inf``.
    ``options``: per-call kernel-variant switches (dict of ``dsge_options`` fields or ``_lib.Options``).
    Returns dict(logp, status[, T, R, resid, n_iter])."""
    check_filter_type(filter_type)

    def hints(a):
        return dict(n_state_hint=state_hint(a["A"]) if n_state_hint is None else n_state_hint,
                    z_selector_hint=selector_hint(a["Z"]) if z_selector_hint is None else z_selector_hint,
                    n_lead_hint=(lead_hint(a["C"], tol) if solver == "gensys" else 0) if n_lead_hint is None else n_lead_hint)

    out = F.solve_kalman_logp(HOST, A, B, C, D, Q, Z, y, d=d, Hdiag=Hdiag, q_mode=q_mode, solver=solver, tol=tol, max_iter=max_iter,
                              jitter=jitter, missing_fill=missing_fill_value, hints=hints, options=options,
                              solver_flags=0 if add_solver_success_check else _lib.SOLVER_FLAG_ZERO_T_ON_FAILURE,
                              return_policy=return_policy)
    return out if return_policy else dict(logp=out["logp"], status=out["status"])


def solve_kalman_logp_grad_batched(A, B, C, D, q, Z, y, d=None, Hdiag=None, solver="cycle_reduction", tol=1e-6, max_iter=50,
                                   jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, n_filter_hint=None,
                                   n_lead_hint=None, options=None, Q=None, dense_z=None, return_Z_bar=False):
    """logp and its reverse-mode gradient per draw (include/dsge_hip.h: dsge_solve_kalman_logp_grad_batched): what
    pytensor autodiff computes for the reference's logp graph, on the device.  ``q``: (k,) or (batch, k) diagonal shock
    variances, or ``q=None, Q=`` a full symmetric shock covariance (k, k) / (batch, k, k) (``full_covariance``,
    statespace.py:247-251); ``Z``: selector design matrix (p, n), p <= 8; n <= 56.
    Returns dict(logp, status, A_bar, B_bar, C_bar, D_bar, q_bar[, d_bar][, h_bar]); with ``Q=`` the key is ``Q_bar``
    (batch, k, k): the cotangent of all k x k entries taken as independent (symmetric).
    A design matrix that is not a selector (observation equations, statespace.py:298-332) takes the dense-Z entry point
    (``dsge_solve_kalman_logp_grad_dense_z_batched``: the observed combinations become p extra variables, n + p <= 56) --
    automatically, or forced with ``dense_z=True``; ``return_Z_bar=True`` adds ``Z_bar`` (batch, p, n), the cotangent of Z."""
    if Q is not None and q is not None:
        raise ValueError("pass either q (diagonal variances) or Q (full covariance)")

    def route(a):
        A, Z, n = a["A"], a["Z"], a["n"]
        dense = (bool(return_Z_bar) or not selector_hint(Z)) if dense_z is None else dense_z
        if n_filter_hint is not None:
            ns = n_filter_hint
        elif dense:  # the dense entry point wants the number of STATE variables (non-zero columns of A in any draw)
            ns = np.count_nonzero(np.any(A.reshape(-1, n) != 0, axis=0))
        else:  # |S u O|: non-zero columns of A (in any draw) or of Z
            ns = np.count_nonzero(np.any(A.reshape(-1, n) != 0, axis=0) | np.any(Z.reshape(-1, n) != 0, axis=0))
        nl = (lead_hint(a["C"], tol) if solver == "gensys" else 0) if n_lead_hint is None else n_lead_hint
        return dict(dense_z=dense, Z_bar=dense and return_Z_bar, n_hint=ns, n_lead_hint=nl)

    out = F.solve_kalman_logp_grad(HOST, A, B, C, D, q if Q is None else Q, Z, y, full=Q is not None, d=d, Hdiag=Hdiag, solver=solver,
                                   tol=tol, max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value, route=route,
                                   options=options)
    if Q is not None:
        out["Q_bar"] = out.pop("q_bar")
    return out


def second_order_structure(A, C, Z):
    """Model structure the second-order path takes as index lists (int32): the state variables S (non-zero columns of A in
    any draw), the forward-looking variables L (non-zero columns of C) and the variables the pruned filter retains, U = S
    followed by the observed non-states (non-zero columns of Z)."""
    A = np.asarray(A)
    C = np.asarray(C)
    n = A.shape[-1]
    S = np.flatnonzero(np.any(A.reshape(-1, n) != 0, axis=0))
    Lc = np.flatnonzero(np.any(C.reshape(-1, n) != 0, axis=0))
    obs = np.flatnonzero(np.any(np.asarray(Z).reshape(-1, n) != 0, axis=0))
    U = np.concatenate([S, np.setdiff1d(obs, S)])
    return S.astype(np.int32), Lc.astype(np.int32), U.astype(np.int32)


def second_order_logp_batched(A, B, C, D, hess_idx, hess_val, q, Z, y, d=None, Hdiag=None, solver="cycle_reduction", tol=1e-8,
                              max_iter=1000, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, return_solution=False,
                              structure=None, options=None):
    """Second-order perturbation + pruned-state-space quasi-likelihood per draw (include/dsge_hip.h:
    ``dsge_second_order_logp_batched``; BASELINE configs[4]).  The reference raises ``NotImplementedError`` for ``order != 1``
    (gEconpy/model/perturbation.py:97-98); this is what replaces the raise.
    ``hess_idx``: (nnz, 3) int32 (equation, z_a <= z_b) sorted by equation, z = [y-; y; y+; u]; ``hess_val``: (batch, nnz);
    ``q``: (k,) or (batch, k) shock variances; ``Z``: (p, n), p <= 8.
    Returns dict(logp, status[, T, R, g_yy (batch, n, s, s), g_yu (batch, n, s, k), g_uu (batch, n, k, k), g_ss (batch, n), S])."""
    out, S = F.second_order_logp(HOST, A, B, C, D, np.asarray(hess_idx).reshape(-1, 3), hess_val, q, Z, y, d=d, Hdiag=Hdiag,
                                 solver=solver, tol=tol, max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value,
                                 structure=second_order_structure if structure is None else structure, options=options,
                                 return_solution=return_solution)
    if not return_solution:
        return dict(logp=out["logp"], status=out["status"])
    return dict(out, S=S)


def simulate_pruned_batched(*args, **kwargs):
    """``simulate_pruned_batched(T, R, g_yy, g_yu, g_uu, g_ss, S, eps, n_steps=None, x0=None, status=None, parts=False)`` -- or, in
    place of the seven solution arguments, the dict ``second_order_logp_batched(..., return_solution=True)`` returns:
    ``simulate_pruned_batched(solution, eps, ...)``.  Simulated paths of the PRUNED second-order system (Kim, Kim, Schaumburg & Sims;
    ``oracle.second_order.simulate_pruned``) for every draw and path at once (include/dsge_hip.h, ``dsge_simulate_pruned_batched``):

        x_f' = T x_f + R u;   x_s' = T x_s + 1/2 g_yy (f (x) f) + g_yu (f (x) u) + 1/2 g_uu (u (x) u) + 1/2 g_ss;   x = x_f + x_s

    with f = x_f[S], in the indexing of ``simulate_batched``: ``eps`` (n_paths, n_shock_steps, k) or (batch, n_paths, n_shock_steps,
    k), ``n_steps`` >= n_shock_steps (later steps carry no shock), ``x0`` None (both parts zero) or a pair ``(xf0, xs0)`` of
    (n_paths, n) or (batch, n_paths, n) arrays, ``status`` optional (batch,) int32 (a non-zero word gives NaN).  Sizes of the
    second-order solver: n <= 64, s <= 24, k <= 12.  Returns dict(x (batch, n_paths, n_steps, n)), with ``parts=True`` also ``x_f``
    and ``x_s`` (``x == x_f + x_s`` to the last bit)."""
    sol, r = F.bind_solution("simulate_pruned_batched", args, kwargs,
                             (("eps", None), ("n_steps", None), ("x0", None), ("status", None), ("parts", False)))
    return F.simulate_pruned(HOST, sol, r["eps"], n_steps=r["n_steps"], x0=r["x0"], status=r["status"], parts=r["parts"])


def girf_pruned_batched(*args, **kwargs):
    """``girf_pruned_batched(T, R, g_yy, g_yu, g_uu, g_ss, S, n_steps=40, impulses=None, eps=None, x0=None, status=None)`` -- or the
    solution dict first, as ``simulate_pruned_batched``.  Generalised impulse responses of the pruned second-order system
    (include/dsge_hip.h, ``dsge_girf_pruned_batched``): impulse j is column j of ``impulses`` ((k, c) or (batch, k, c); default
    ``I_k``), added to the first shock of every baseline path of ``eps`` ((n_paths, n_shock_steps, k) or batched; None: one path
    without shocks, the deterministic response from ``x0``), and

        girf[b, j, t] = mean over paths p of  x_t(path p with the impulse) - x_t(path p)

    summed in ascending path order, reproducible bit for bit.  Its first-order part is ``impulse_response_batched(T, R, S=impulses)``;
    the rest depends on the state, the sign and the size of the impulse.  Returns dict(girf (batch, c, n_steps, n))."""
    sol, r = F.bind_solution("girf_pruned_batched", args, kwargs,
                             (("n_steps", 40), ("impulses", None), ("eps", None), ("x0", None), ("status", None)))
    return dict(girf=F.girf_pruned(HOST, sol, n_steps=r["n_steps"], impulses=r["impulses"], eps=r["eps"], x0=r["x0"],
                                   status=r["status"]))
