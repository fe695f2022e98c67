"""The front-end of the entry points that exist for host arrays (``batched.*_batched``) AND for device tensors (``LogpEngine``),
written once: shapes and layouts are read off ``.shape`` (numpy array or torch tensor alike), outputs are allocated or reused,
the arguments are named once and handed to ``_lib.call``.

A backend ``b`` is what differs between the two: ``b.inp(x, dtype)`` coerces (host) or checks (device) an input, ``b.empty(shape,
dtype)`` allocates an output, ``b.ptr(x)`` takes its address, ``b.host`` / ``b.stream`` pick the host twin or the stream, and
``b.status_io(status, nb)`` is the in/out status word of a filter (fresh zeros by default).  ``HOST`` is the numpy one; the torch one
lives in engine.py (this module never imports torch).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

Q_MODES = {"diag": _lib.Q_DIAG_SHARED, "diag_batched": _lib.Q_DIAG_BATCHED, "full": _lib.Q_FULL_SHARED,
           "full_batched": _lib.Q_FULL_BATCHED}


class HostBackend:
    host, stream = True, None

    @staticmethod
    def inp(x, dtype="float64"):
        return None if x is None else np.ascontiguousarray(x, dtype=dtype)

    @staticmethod
    def empty(shape, dtype="float64"):
        return np.empty(shape, dtype=dtype)

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def status_io(status, nb):
        return np.zeros(nb, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32).copy()

    # what the generated draws of ``simulation_smoother`` need: the array module, standard normals from ``rng`` (a seed or a
    # ``np.random.Generator``), and the symmetric-eigen factor S S' = A of a stack of positive semi-definite matrices
    xp = np

    @staticmethod
    def generator(rng):
        return np.random.default_rng(rng)

    @staticmethod
    def randn(gen, shape):
        return gen.standard_normal(shape)

    @staticmethod
    def sym_factor(A):
        w, V = np.linalg.eigh(np.where(np.isfinite(A), A, 0.0))  # (a failed draw's matrix: its outputs are NaN by its status)
        return np.ascontiguousarray(V * np.sqrt(np.clip(w, 0.0, None))[..., None, :])


HOST = HostBackend()


# ---- shapes and layouts ----------------------------------------------------------------------------------------------------------
def q_layout(shape, q_mode, nb, k):
    """The layout code of a shock covariance of this shape: named by ``q_mode`` (a key of ``Q_MODES`` or the code itself) and
    checked, or inferred (ambiguous only when batch == k)."""
    shape = tuple(shape)
    want = {_lib.Q_DIAG_SHARED: (k,), _lib.Q_DIAG_BATCHED: (nb, k), _lib.Q_FULL_SHARED: (k, k), _lib.Q_FULL_BATCHED: (nb, k, k)}
    if q_mode is None:
        codes = [code for code, s in want.items() if s == shape]
        if len(codes) != 1:
            raise ValueError(f"cannot infer the layout of Q with shape {shape} (batch={nb}, k={k}); pass q_mode")
        return codes[0]
    code = Q_MODES[q_mode] if isinstance(q_mode, str) else int(q_mode)
    if shape != want[code]:
        raise ValueError(f"Q has shape {shape}, q_mode needs {want[code]}")
    return code


def grad_q_layout(shape, full, nb, k):
    """The gradient and second-order entries are told whether the covariance is full; the shape says whether it is batched."""
    shape = tuple(shape)
    if full:
        if shape not in ((k, k), (nb, k, k)):
            raise ValueError("Q must be (k, k) or (batch, k, k)")
        return _lib.Q_FULL_SHARED + (len(shape) == 3)
    if shape not in ((k,), (nb, k)):
        raise ValueError("q must be (k,) or (batch, k) (diagonal shock covariance)")
    return int(len(shape) == 2)


def shared_or_batched(x, nb, tail, name, says=None):
    """0 for ``x`` of shape ``tail`` (shared by all draws), 1 for ``(batch,) + tail``."""
    shape, tail = tuple(x.shape), tuple(tail)
    if shape == tail:
        return 0
    if shape == (nb, *tail):
        return 1
    raise ValueError(f"{name} must be {says or f'{tail} or {(nb, *tail)}'}; got {shape}")


def obs_flags(Z, d, Hdiag, nb, p, m):
    """(z_batched, d_batched, h_batched) of the observation model ``y = Z x + d + N(0, diag(Hdiag))``; d, Hdiag may be None."""
    return (shared_or_batched(Z, nb, (p, m), "Z", "(p, m) or (batch, p, m)"),
            *(0 if x is None else shared_or_batched(x, nb, (p,), name, "(p,) or (batch, p)") for x, name in ((d, "d"), (Hdiag, "Hdiag"))))


def check_status(st, nb):
    if st is not None and tuple(st.shape) != (nb,):
        raise ValueError(f"status must be (batch,); got {tuple(st.shape)}")
    return st


def cov_flags(covariances):
    """``covariances`` = "diag" / "full" / None -> (covariances wanted, full matrices)."""
    if covariances not in ("diag", "full", None):
        raise ValueError('covariances must be "diag", "full" or None')
    return covariances is not None, covariances == "full"


def _nd(x, ndim):
    if x.ndim != ndim:
        raise ValueError(f"expected a {ndim}-d array, got shape {tuple(x.shape)}")
    return x


def _is(x, shape, name, says=None):
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must be {says or tuple(shape)}; got {tuple(x.shape)}")
    return x


def check_abc(b, A, B, C):
    A, B, C = (_nd(b.inp(x), 3) for x in (A, B, C))
    if not (A.shape == B.shape == C.shape and A.shape[1] == A.shape[2]):
        raise ValueError(f"A, B, C must be (batch, n, n); got {tuple(A.shape)}, {tuple(B.shape)}, {tuple(C.shape)}")
    return A, B, C


def model_args(b, A, B, C, D, y):
    """The inputs every fused entry takes first -> the named arguments they make."""
    A, B, C = check_abc(b, A, B, C)
    D, y = _nd(b.inp(D), 3), _nd(b.inp(y), 2)
    nb, n, _ = A.shape
    _is(D, (nb, n, D.shape[2]), "D", "(batch, n, k)")
    return dict(A=A, B=B, C=C, D=D, y=y, batch=nb, n=n, k=D.shape[2], p=y.shape[1], T_len=y.shape[0])


def obs_args(b, Z, d, Hdiag, nb, p, m):
    Z, d, Hdiag = b.inp(Z), b.inp(d), b.inp(Hdiag)
    zb, db, hb = obs_flags(Z, d, Hdiag, nb, p, m)
    return dict(Z=Z, z_batched=zb, d=d, d_batched=db, Hdiag=Hdiag, h_batched=hb)


def _TR(b, T, R, name, smoother=False):
    T, R = _nd(b.inp(T), 3), _nd(b.inp(R), 3)
    nb, m, m2 = T.shape
    if m != m2 or tuple(R.shape[:2]) != (nb, m) or (R.shape[2] < 1 and not smoother):
        raise ValueError(f"T must be (batch, m, m) and R (batch, m, k); got {tuple(T.shape)}, {tuple(R.shape)}")
    cap = _lib.MAX_N if smoother else _lib.MAX_N_BIG
    if m > cap:
        raise ValueError(f"{name}: m = {m}, {'the smoother takes ' if smoother else ''}at most {cap} variables")
    return T, R, nb, m, R.shape[2]


def _out(b, given, shape, dtype="float64"):
    """An output buffer: ``given`` (checked) or a fresh one."""
    return b.empty(shape, dtype) if given is None else _is(b.inp(given, dtype), shape, "an output buffer")


def call(b, entry, **named):
    """``_lib.call`` for backend ``b``: a POINTER argument (by the table, not by the look of the value) that is not an address
    already (None or an int) is a buffer of the backend."""
    pointers = {name for name, kind in _lib.SIGNATURES[entry] if kind is ctypes.c_void_p}
    _lib.call(entry, host=b.host, stream=b.stream,
              **{key: b.ptr(v) if key in pointers and not (v is None or isinstance(v, int)) else v for key, v in named.items()})


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def solve_kalman_logp(b, A, B, C, D, Q, Z, y, *, d, Hdiag, q_mode, solver, tol, max_iter, jitter, missing_fill, hints, options,
                      solver_flags=0, return_policy=False, out=None):
    """``hints(a)``: the named hint arguments, from the validated arguments ``a``.  ``out``: buffers to reuse (logp, status, T, R)."""
    a = model_args(b, A, B, C, D, y)
    nb, n, k = a["batch"], a["n"], a["k"]
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    a.update(obs_args(b, Z, d, Hdiag, nb, a["p"], n))
    out = out or {}
    res = dict(logp=_out(b, out.get("logp"), (nb,)), status=_out(b, out.get("status"), (nb,), "int32"))
    for key, shape, dtype in (("T", (nb, n, n), "float64"), ("R", (nb, n, k), "float64"), ("resid", (nb,), "float64"),
                              ("n_iter", (nb,), "int32")):
        res[key] = _out(b, out.get(key), shape, dtype) if return_policy or out.get(key) is not None else None
    op, _keep = _lib.opt_ptr(options)
    call(b, "dsge_solve_kalman_logp_batched_opt", opt=op, **a, Q=Q, q_mode=code, solver=_lib.SOLVER_CODES[solver] | solver_flags,
         tol=tol, max_iter=max_iter, jitter=jitter, missing_fill=missing_fill, **hints(a), logp_out=res["logp"],
         status_out=res["status"], T_out=res["T"], R_out=res["R"], resid_out=res["resid"], n_iter_out=res["n_iter"])
    return res


def solve_kalman_logp_grad(b, A, B, C, D, q, Z, y, *, full, d, Hdiag, solver, tol, max_iter, jitter, missing_fill, route, options,
                           out=None):
    """``full``: ``q`` is a full covariance.  ``route(a)`` -> dict(dense_z, Z_bar (wanted), n_hint, n_lead_hint).  ``out``: the dict
    of an earlier call, completed in place."""
    a = model_args(b, A, B, C, D, y)
    nb, n, k, p = a["batch"], a["n"], a["k"], a["p"]
    q = b.inp(q)
    qb = grad_q_layout(q.shape, full, nb, k)
    a.update(obs_args(b, Z, d, Hdiag, nb, p, n))
    r = route(a)
    res = {} if out is None else out
    for key, shape, wanted in (("logp", (nb,), True), ("status", (nb,), True), ("A_bar", (nb, n, n), True), ("B_bar", (nb, n, n), True),
                               ("C_bar", (nb, n, n), True), ("D_bar", (nb, n, k), True), ("q_bar", (nb, k, k) if full else (nb, k), True),
                               ("d_bar", (nb, p), d is not None), ("h_bar", (nb, p), Hdiag is not None), ("Z_bar", (nb, p, n), r["Z_bar"])):
        if wanted or res.get(key) is not None:
            res[key] = _out(b, res.get(key), shape, "int32" if key == "status" else "float64")
    named = dict(a, q=q, q_batched=qb, solver=_lib.SOLVER_CODES[solver], tol=tol, max_iter=max_iter, jitter=jitter,
                 missing_fill=missing_fill, n_lead_hint=r["n_lead_hint"], logp_out=res["logp"], status_out=res["status"],
                 d_bar=res.get("d_bar"), h_bar=res.get("h_bar"), **{key: res[key] for key in ("A_bar", "B_bar", "C_bar", "D_bar", "q_bar")})
    if r["dense_z"]:
        with _lib.options_scope(options):
            call(b, "dsge_solve_kalman_logp_grad_dense_z_batched", **named, n_state_hint=r["n_hint"], Z_bar=res.get("Z_bar"))
    else:
        op, _keep = _lib.opt_ptr(options)
        call(b, "dsge_solve_kalman_logp_grad_batched_opt", opt=op, **named, n_filter_hint=r["n_hint"])
    return res


def second_order_logp(b, A, B, C, D, hess_idx, hess_val, q, Z, y, *, d, Hdiag, solver, tol, max_iter, jitter, missing_fill, structure,
                      options, return_solution=False, out=None, stage_ms=None):
    """``structure``: (S, L, U) index lists, or the function of the validated (A, C, Z) that makes them.  Returns the outputs and S."""
    a = model_args(b, A, B, C, D, y)
    nb, n, k, p = a["batch"], a["n"], a["k"], a["p"]
    hess_idx = _nd(b.inp(hess_idx, "int32"), 2)
    nnz = hess_idx.shape[0]
    _is(hess_idx, (nnz, 3), "hess_idx", "(nnz, 3)")
    hess_val = _is(_nd(b.inp(hess_val), 2), (nb, nnz), "hess_val", "(batch, nnz)")
    q = b.inp(q)
    qb = grad_q_layout(q.shape, False, nb, k)
    Z = _is(_nd(b.inp(Z), 2), (p, n), "Z", "(p, n)")
    d, Hdiag = (None if x is None else _is(_nd(b.inp(x), 1), (p,), name, "(p,)") for x, name in ((d, "d"), (Hdiag, "Hdiag")))
    S, Lc, U = (np.ascontiguousarray(x, dtype=np.int32) for x in (structure(a["A"], a["C"], Z) if callable(structure) else structure))
    s = len(S)
    out = out or {}
    res = dict(logp=_out(b, out.get("logp"), (nb,)), status=_out(b, out.get("status"), (nb,), "int32"))
    for key, shape in (("T", (nb, n, n)), ("R", (nb, n, k)), ("g_yy", (nb, n, s, s)), ("g_yu", (nb, n, s, k)), ("g_uu", (nb, n, k, k)),
                       ("g_ss", (nb, n))):
        res[key] = b.empty(shape) if return_solution else None
    with _lib.options_scope(options):
        call(b, "dsge_second_order_logp_batched", **a, hess_idx=hess_idx, nnz=nnz, hess_val=hess_val, q=q, q_batched=qb, Z=Z, d=d,
             Hdiag=Hdiag, solver=_lib.SOLVER_CODES[solver], tol=tol, max_iter=max_iter, jitter=jitter, missing_fill=missing_fill,
             state_idx=S.ctypes.data, n_state=s, lead_idx=Lc.ctypes.data, n_lead=len(Lc), ret_idx=U.ctypes.data, n_ret=len(U),
             logp_out=res["logp"], status_out=res["status"], T_out=res["T"], R_out=res["R"], gyy_out=res["g_yy"], gyu_out=res["g_yu"],
             guu_out=res["g_uu"], gss_out=res["g_ss"], stage_ms=stage_ms)
    return res, S


def kalman_smoother(b, name, T, R, Q, Z, y, *, d, Hdiag, q_mode, status, jitter, missing_fill, cov, full, rank_tol, scratch_limit_bytes,
                    options):
    """``cov`` / ``full``: covariances wanted / as full matrices."""
    T, R, nb, m, k = _TR(b, T, R, name, smoother=True)
    y = _nd(b.inp(y), 2)
    T_len, p = y.shape
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    obs = obs_args(b, Z, d, Hdiag, nb, p, m)
    limit = 0 if scratch_limit_bytes is None else int(scratch_limit_bytes)
    if limit < 0:
        raise ValueError("scratch_limit_bytes must be >= 0")
    st = check_status(b.status_io(status, nb), nb)
    res = dict(ll=b.empty((nb, T_len)), smoothed_states=b.empty((nb, T_len, m)),
               smoothed_covs=b.empty((nb, T_len, m, m) if full else (nb, T_len, m)) if cov else None,
               smoothed_shocks=b.empty((nb, T_len, k)), status=st)
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        call(b, "dsge_kalman_smoother_batched", T=T, R=R, Q=Q, q_mode=code, **obs, y=y, batch=nb, m=m, k=k, p=p, T_len=T_len,
             jitter=jitter, missing_fill=missing_fill, rank_tol=0.0 if rank_tol is None else rank_tol, scratch_limit_bytes=limit,
             ll_out=res["ll"], a_smooth_out=res["smoothed_states"], p_smooth_out=res["smoothed_covs"],
             eps_smooth_out=res["smoothed_shocks"], full_cov=bool(full), status_io=st)
    return res


def simulation_smoother_scratch_bytes_per_draw(m, T_len, n_paths):
    """``2 T_len m^2 + 2 T_len m`` doubles of the stored forward pass and ``3 n_paths T_len m`` of the paths (x+, a*_pred, a*_filt)."""
    return 8 * (2 * T_len * m * m + 2 * T_len * m + 3 * n_paths * T_len * m)


def stationary_factor(b, name, T, R, Q, *, q_mode):
    """F (batch, m, m) with F F' = P0 = dlyap(T, R Q R') (``dsge_lyapunov_batched``), F = V sqrt(max(lambda, 0)) from a float64
    symmetric eigendecomposition."""
    T, R, nb, m, k = _TR(b, T, R, name, smoother=True)
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    P0, RQR, st = b.empty((nb, m, m)), b.empty((nb, m, m)), b.empty((nb,), "int32")
    call(b, "dsge_lyapunov_batched", T=T, R=R, Q=Q, q_mode=code, batch=nb, m=m, k=k, P0_out=P0, RQR_out=RQR, status=st)
    return b.sym_factor(0.5 * (P0 + b.xp.swapaxes(P0, -1, -2)))


def _path_array(b, x, nb, tail, name):
    """A draw array: None, ``tail`` (shared by all draws) or ``(batch,) + tail`` -> (array, batched flag)."""
    x = b.inp(x)
    return (None, 0) if x is None else (x, shared_or_batched(x, nb, tail, name))


def simulation_smoother(b, name, T, R, Q, Z, y, *, n_paths, d, Hdiag, q_mode, x0, eps, eta, rng, return_draws, status, jitter,
                        missing_fill, rank_tol, scratch_limit_bytes, options):
    """``rng``: what ``b.generator`` takes (host: a seed or ``np.random.Generator``; device: a ``torch.Generator`` or None)."""
    T, R, nb, m, k = _TR(b, T, R, name, smoother=True)
    y = _nd(b.inp(y), 2)
    T_len, p = y.shape
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    obs = obs_args(b, Z, d, Hdiag, nb, p, m)
    n_paths = int(n_paths)
    if n_paths < 1:
        raise ValueError(f"n_paths must be >= 1; got {n_paths}")
    if eta is not None and Hdiag is None:
        raise ValueError("eta (a measurement-noise draw) needs Hdiag")
    x0, xb = _path_array(b, x0, nb, (n_paths, m), "x0")
    eps, eb = _path_array(b, eps, nb, (n_paths, T_len, k), "eps")
    eta, hb = _path_array(b, eta, nb, (n_paths, T_len, p), "eta")
    limit = 0 if scratch_limit_bytes is None else int(scratch_limit_bytes)
    if limit < 0:
        raise ValueError("scratch_limit_bytes must be >= 0")
    st = check_status(b.status_io(status, nb), nb)
    # the draws nobody passed, from standard normals: eps = z sqrt(q) or z S' (S S' = Q), eta = z sqrt(H), x0 = z F' (F F' = P0)
    xp = b.xp
    gen = b.generator(rng) if (x0 is None or eps is None or (eta is None and Hdiag is not None)) else None
    if x0 is None:
        F = stationary_factor(b, name, T, R, Q, q_mode=code)
        x0, xb = xp.matmul(b.randn(gen, (nb, n_paths, m)), xp.swapaxes(F, -1, -2)), 1
    if eps is None:
        z = b.randn(gen, (nb, n_paths, T_len, k))
        if code in (_lib.Q_DIAG_SHARED, _lib.Q_DIAG_BATCHED):
            eps = z * xp.sqrt(Q).reshape(-1, 1, 1, k)
        else:
            eps = xp.matmul(z, xp.swapaxes(b.sym_factor(Q), -1, -2).reshape(-1, 1, k, k))
        eb = 1
    if eta is None and Hdiag is not None:
        eta, hb = b.randn(gen, (nb, n_paths, T_len, p)) * xp.sqrt(obs["Hdiag"]).reshape(-1, 1, 1, p), 1
    x0, eps, eta = (None if v is None else b.inp(v if b.host else v.contiguous()) for v in (x0, eps, eta))
    res = dict(states=b.empty((nb, n_paths, T_len, m)), shocks=b.empty((nb, n_paths, T_len, k)), ll=b.empty((nb, T_len)), status=st)
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        call(b, "dsge_simulation_smoother_batched", T=T, R=R, Q=Q, q_mode=code, **obs, y=y, batch=nb, m=m, k=k, p=p, T_len=T_len,
             jitter=jitter, missing_fill=missing_fill, rank_tol=0.0 if rank_tol is None else rank_tol, scratch_limit_bytes=limit,
             x0=x0, x0_batched=xb, eps=eps, eps_batched=eb, eta=eta, eta_batched=hb, n_paths=n_paths, ll_out=res["ll"],
             x_out=res["states"], eps_out=res["shocks"], status_io=st)
    if return_draws:
        res.update(x0=x0, eps=eps, eta=eta)
    return res


def simulate(b, name, T, R, eps, *, n_steps, x0, status, out=None):
    T, R, nb, m, k = _TR(b, T, R, name)
    eps = b.inp(eps)
    if eps.ndim not in (3, 4) or eps.shape[-1] != k:
        raise ValueError(f"eps must be (n_paths, n_shock_steps, {k}) or (batch, n_paths, n_shock_steps, {k}); got {tuple(eps.shape)}")
    n_paths, n_shock = eps.shape[-3], eps.shape[-2]
    eb = shared_or_batched(eps, nb, (n_paths, n_shock, k), "eps")
    n_steps = n_shock if n_steps is None else int(n_steps)
    if n_steps < n_shock:
        raise ValueError(f"n_steps = {n_steps} is less than the {n_shock} shock steps of eps")
    x0 = b.inp(x0)
    xb = 0 if x0 is None else shared_or_batched(x0, nb, (n_paths, m), "x0")
    st = check_status(b.inp(status, "int32"), nb)
    paths = _out(b, out, (nb, n_paths, n_steps, m))
    call(b, "dsge_simulate_batched", T=T, R=R, eps=eps, eps_batched=eb, x0=x0, x0_batched=xb, status=st, batch=nb, m=m, k=k,
         n_paths=n_paths, n_steps=n_steps, n_shock_steps=n_shock, x_out=paths)
    return paths


def impulse_response(b, name, T, R, *, n_steps, S, weights, fevd, irf, status, out=None):
    T, R, nb, m, k = _TR(b, T, R, name)
    sb, c = 0, k
    if S is not None:
        S = b.inp(S)
        if S.ndim not in (2, 3) or S.shape[-2] != k:
            raise ValueError(f"S must be ({k}, c) or (batch, {k}, c); got {tuple(S.shape)}")
        c = S.shape[-1]
        sb = shared_or_batched(S, nb, (k, c), "S")
    weights = b.inp(weights)
    wb = 0 if weights is None else shared_or_batched(weights, nb, (c,), "weights")
    if not (irf or fevd):
        raise ValueError("nothing requested: irf and fevd are both off")
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError("n_steps must be >= 0")
    st = check_status(b.inp(status, "int32"), nb)
    out = out or {}
    res = dict(irf=_out(b, out.get("irf"), (nb, c, n_steps, m)) if irf else None,
               fevd=_out(b, out.get("fevd"), (nb, n_steps, m, c)) if fevd else None)
    call(b, "dsge_irf_batched", T=T, R=R, S=S, s_batched=sb, weights=weights, w_batched=wb, status=st, batch=nb, m=m, k=k, c=c,
         n_steps=n_steps, irf_out=res["irf"], fevd_out=res["fevd"])
    return res


def forecast(b, name, T, R, Q, a0, *, P0, n_steps, Z, d, Hdiag, q_mode, covariances, status, out=None):
    T, R, nb, m, k = _TR(b, T, R, name)
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    a0 = _is(b.inp(a0), (nb, m), "a0")
    P0 = None if P0 is None else _is(b.inp(P0), (nb, m, m), "P0")
    cov, full = cov_flags(covariances)
    p, obs = 0, dict(Z=None, z_batched=0, d=None, d_batched=0, Hdiag=None, h_batched=0)
    if Z is not None:
        Z = b.inp(Z)
        p = Z.shape[-2] if Z.ndim >= 2 else 0
        obs = obs_args(b, Z, d, Hdiag, nb, p, m)
    elif d is not None or Hdiag is not None:
        raise ValueError("d and Hdiag need Z")
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError("n_steps must be >= 0")
    st = check_status(b.inp(status, "int32"), nb)
    out = out or {}
    res = dict(states=_out(b, out.get("states"), (nb, n_steps, m)),
               covs=_out(b, out.get("covs"), (nb, n_steps, m, m) if full else (nb, n_steps, m)) if cov else None,
               observed=_out(b, out.get("observed"), (nb, n_steps, p)) if p else None,
               observed_covs=_out(b, out.get("observed_covs"), (nb, n_steps, p, p)) if p and cov else None)
    call(b, "dsge_forecast_batched", T=T, R=R, Q=Q, q_mode=code, **obs, a0=a0, P0=P0, status=st, batch=nb, m=m, k=k, p=p,
         n_steps=n_steps, a_out=res["states"], p_out=res["covs"], full_cov=full, y_out=res["observed"], f_out=res["observed_covs"])
    return res


SEGMENT_OUTPUTS = ("logp", "ll", "a_last", "P_last")


def segment_starts(seg_start, T_len):
    """The dated breaks as the library takes them -- a HOST int32 list with seg_start[0] == 0, strictly increasing, every entry
    < T_len (when T_len > 0), 1 .. ``_lib.MAX_SEGMENTS`` entries -- checked as ``check_kalman_segments`` (csrc/dsge_host.hpp) checks."""
    if seg_start is None:
        raise ValueError("seg_start is required")
    raw = np.asarray(seg_start)
    if raw.ndim != 1 or (raw.size and raw.dtype.kind not in "iu"):
        raise ValueError("seg_start must be a 1-d list of integers")
    seg = np.ascontiguousarray(raw, dtype=np.int32)
    if not 1 <= seg.size <= _lib.MAX_SEGMENTS:
        raise ValueError(f"seg_start has {seg.size} entries; 1 .. {_lib.MAX_SEGMENTS} segments")
    if seg[0] != 0:
        raise ValueError("seg_start[0] must be 0")
    if np.any(np.diff(seg) <= 0):
        raise ValueError("seg_start must be strictly increasing")
    if T_len > 0 and seg[-1] >= T_len:
        raise ValueError(f"seg_start: every entry must be < T_len = {T_len}")
    return seg


def segment_q_layout(shape, q_mode, nb, S, k):
    """``q_layout`` with a segment axis behind the draw axis: (S, k), (batch, S, k), (S, k, k) or (batch, S, k, k)."""
    shape = tuple(shape)
    want = {_lib.Q_DIAG_SHARED: (S, k), _lib.Q_DIAG_BATCHED: (nb, S, k), _lib.Q_FULL_SHARED: (S, k, k), _lib.Q_FULL_BATCHED: (nb, S, k, k)}
    if q_mode is None:
        codes = [code for code, w in want.items() if w == shape]
        if len(codes) != 1:
            raise ValueError(f"cannot infer the layout of Q with shape {shape} (batch={nb}, segments={S}, k={k}); pass q_mode")
        return codes[0]
    code = Q_MODES[q_mode] if isinstance(q_mode, str) else int(q_mode)
    if shape != want[code]:
        raise ValueError(f"Q has shape {shape}, q_mode needs {want[code]}")
    return code


def _segment_inputs(b, name, T, R, Q, Z, y, seg_start, Hdiag, d, a0, P0, shift, q_mode):
    """The inputs the entries across dated breaks share, validated -> the named arguments they make (``T`` .. ``T_len``)."""
    T, R = b.inp(T), b.inp(R)
    if T is None or R is None or Q is None or Z is None or y is None:
        raise ValueError(f"{name}: T, R, Q, Z and y are required")
    T, R, y = _nd(T, 4), _nd(R, 4), _nd(b.inp(y), 2)
    nb, S, m, m2 = T.shape
    k = R.shape[3]
    if m != m2 or m < 1 or tuple(R.shape[:3]) != (nb, S, m) or k < 1:
        raise ValueError(f"T must be (batch, S, m, m) and R (batch, S, m, k); got {tuple(T.shape)}, {tuple(R.shape)}")
    T_len, p = y.shape
    seg = segment_starts(seg_start, T_len)
    if seg.size != S:
        raise ValueError(f"seg_start has {seg.size} entries, T has {S} segments")
    Q = b.inp(Q)
    code = segment_q_layout(Q.shape, q_mode, nb, S, k)
    Z, d, Hdiag = b.inp(Z), b.inp(d), b.inp(Hdiag)
    zb = shared_or_batched(Z, nb, (S, p, m), "Z", "(S, p, m) or (batch, S, p, m)")
    db, hb = (0 if x is None else shared_or_batched(x, nb, (S, p), nm, "(S, p) or (batch, S, p)") for x, nm in ((d, "d"), (Hdiag, "Hdiag")))
    a0 = None if a0 is None else _is(b.inp(a0), (nb, m), "a0")
    P0 = None if P0 is None else _is(b.inp(P0), (nb, m, m), "P0")
    shift = None if shift is None else _is(b.inp(shift), (nb, S, m), "shift", "(batch, S, m)")
    # (``_seg``: keeps the host list alive for the call)
    return dict(T=T, R=R, Q=Q, q_mode=code, Z=Z, z_batched=zb, d=d, d_batched=db, Hdiag=Hdiag, h_batched=hb, a0=a0, P0=P0, shift=shift,
                y=y, seg_start=seg.ctypes.data, n_seg=S, batch=nb, m=m, k=k, p=p, T_len=T_len), seg


def kalman_logp_segments(b, name, T, R, Q, Z, y, seg_start, *, Hdiag, d, a0, P0, shift, q_mode, status, jitter, missing_fill, options,
                         outputs=SEGMENT_OUTPUTS, out=None):
    """``dsge_kalman_logp_segments_batched``: T (batch, S, m, m), R (batch, S, m, k), every other per-segment array with the segment
    axis behind the draw axis.  ``outputs``: which of ``SEGMENT_OUTPUTS`` are computed (logp always is); ``out``: buffers to reuse."""
    a, _seg = _segment_inputs(b, name, T, R, Q, Z, y, seg_start, Hdiag, d, a0, P0, shift, q_mode)
    nb, m, T_len = a["batch"], a["m"], a["T_len"]
    outputs = tuple(outputs)
    if not set(outputs) <= set(SEGMENT_OUTPUTS):
        raise ValueError(f"outputs must be among {SEGMENT_OUTPUTS}; got {outputs}")
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    res = dict(logp=_out(b, out.get("logp"), (nb,)), status=st)
    for key, shape in (("ll", (nb, T_len)), ("a_last", (nb, m)), ("P_last", (nb, m, m))):
        res[key] = _out(b, out.get(key), shape) if key in outputs or out.get(key) is not None else None
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        call(b, "dsge_kalman_logp_segments_batched", **a, jitter=jitter, missing_fill=missing_fill, logp_out=res["logp"],
             ll_out=res["ll"], a_last_out=res["a_last"], P_last_out=res["P_last"], status_io=st)
    return res


SEGMENT_SMOOTHER_OUTPUTS = ("ll", "a_pred", "a_filt", "P_pred", "P_filt", "smoothed_states", "smoothed_covs", "smoothed_shocks")
_SEGMENT_SMOOTHER_ARGS = dict(ll="ll_out", a_pred="a_pred_out", a_filt="a_filt_out", P_pred="p_pred_out", P_filt="p_filt_out",
                              smoothed_states="a_smooth_out", smoothed_covs="p_smooth_out", smoothed_shocks="eps_smooth_out")


def segment_smoother_scratch_bytes_per_draw(m, T_len, n_seg):
    """What ``scratch_limit_bytes`` counts per draw: ``2 T_len m^2 + 2 T_len m`` doubles of the stored forward pass and the
    ``3 n_seg`` basis images (``ks_mat(m)``: 16 ceil(m / 16) rows of two doubles more)."""
    mp = 16 * ((m + 15) // 16)
    return 8 * (2 * T_len * m * m + 2 * T_len * m + 3 * n_seg * mp * (mp + 2))


def kalman_smoother_segments(b, name, T, R, Q, Z, y, seg_start, *, Hdiag, d, a0, P0, shift, q_mode, status, jitter, missing_fill, full,
                             rank_tol, scratch_limit_bytes, options, outputs=SEGMENT_SMOOTHER_OUTPUTS, out=None):
    """``dsge_kalman_smoother_segments_batched``: the inputs of ``kalman_logp_segments``.  ``outputs``: which of
    ``SEGMENT_SMOOTHER_OUTPUTS`` are computed (at least one; without "smoothed_covs" the covariance recursion is skipped); ``full``:
    covariances as full matrices; ``out``: buffers to reuse."""
    a, _seg = _segment_inputs(b, name, T, R, Q, Z, y, seg_start, Hdiag, d, a0, P0, shift, q_mode)
    nb, m, k, T_len = a["batch"], a["m"], a["k"], a["T_len"]
    if m > _lib.MAX_N:
        raise ValueError(f"{name}: m = {m}, the smoother takes at most {_lib.MAX_N} variables")
    out = out or {}
    outputs = tuple(outputs)
    if not set(outputs) <= set(SEGMENT_SMOOTHER_OUTPUTS):
        raise ValueError(f"outputs must be among {SEGMENT_SMOOTHER_OUTPUTS}; got {outputs}")
    if not outputs and all(out.get(key) is None for key in SEGMENT_SMOOTHER_OUTPUTS):
        raise ValueError(f"{name}: at least one output is required")
    limit = 0 if scratch_limit_bytes is None else int(scratch_limit_bytes)
    if limit < 0:
        raise ValueError("scratch_limit_bytes must be >= 0")
    st = check_status(b.status_io(status, nb), nb)
    cov = (nb, T_len, m, m) if full else (nb, T_len, m)
    shapes = dict(ll=(nb, T_len), a_pred=(nb, T_len, m), a_filt=(nb, T_len, m), P_pred=cov, P_filt=cov, smoothed_states=(nb, T_len, m),
                  smoothed_covs=cov, smoothed_shocks=(nb, T_len, k))
    res = {key: _out(b, out.get(key), shape) if key in outputs or out.get(key) is not None else None for key, shape in shapes.items()}
    res["status"] = st
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        call(b, "dsge_kalman_smoother_segments_batched", **a, jitter=jitter, missing_fill=missing_fill,
             rank_tol=0.0 if rank_tol is None else rank_tol, scratch_limit_bytes=limit, full_cov=bool(full), status_io=st,
             **{arg: res[key] for key, arg in _SEGMENT_SMOOTHER_ARGS.items()})
    return res


def _or_over_segments(b, st, nb, S):
    """The status words of the flattened (draw, segment) problems ORed per draw -> a fresh contiguous int32 (batch,) of the backend
    (neither numpy nor torch reduces with a bitwise OR under one name: the at most 8 columns are folded)."""
    st2 = st.reshape(nb, S)
    acc = st2[:, 0] * 1
    for s in range(1, S):
        acc = acc | st2[:, s]
    return b.inp(acc if b.host else acc.contiguous(), "int32")


def _solve_segments(b, name, A, B, C, D, Q, Z, y, seg_start, solver, tol, max_iter, n_lead_hint, options):
    """A .. D (batch, S, n, n | k): every (draw, segment) solved by the EXISTING solver entry on the flattened batch, the segments'
    status words ORed per draw (array operations of the backend: no host round trip on the device).  Returns T (batch, S, n, n),
    R (batch, S, n, k) and the status (batch,)."""
    A, B, C, D = (b.inp(x) for x in (A, B, C, D))
    if any(x is None for x in (A, B, C, D, Q, Z, y)):
        raise ValueError(f"{name}: A, B, C, D, Q, Z and y are required")
    A, D = _nd(A, 4), _nd(D, 4)
    nb, S, n, n2 = A.shape
    k = D.shape[3]
    if n != n2 or tuple(B.shape) != tuple(A.shape) or tuple(C.shape) != tuple(A.shape) or tuple(D.shape[:3]) != (nb, S, n) or k < 1:
        raise ValueError(f"A, B, C must be (batch, S, n, n) and D (batch, S, n, k); got {tuple(A.shape)}, {tuple(B.shape)}, "
                         f"{tuple(C.shape)}, {tuple(D.shape)}")
    if solver not in ("cycle_reduction", "gensys", "backward_direct"):
        raise ValueError(f"solver must be cycle_reduction, gensys or backward_direct; got {solver!r}")
    segment_starts(seg_start, _nd(b.inp(y), 2).shape[0])  # (refused before the solver runs)
    flat = nb * S
    Af, Bf, Cf, Df = A.reshape(flat, n, n), B.reshape(flat, n, n), C.reshape(flat, n, n), D.reshape(flat, n, k)
    T, R, st = b.empty((flat, n, n)), b.empty((flat, n, k)), b.empty((flat,), "int32")
    with _lib.options_scope(options):
        if solver == "cycle_reduction":
            call(b, "dsge_cycle_reduction_batched", A=Af, B=Bf, C=Cf, batch=flat, n=n, max_iter=max_iter, tol=tol, T_out=T, status=st,
                 n_iter=None)
            call(b, "dsge_selection_batched", A=None, B=Bf, C=Cf, D=Df, T=T, batch=flat, n=n, k=k, R_out=R, resid_out=None)
        elif solver == "gensys":
            eu = b.empty((flat, 3), "int32")
            call(b, "dsge_gensys_batched", A=Af, B=Bf, C=Cf, D=Df, batch=flat, n=n, k=k, tol=tol, n_lead_hint=n_lead_hint, T_out=T,
                 R_out=R, eu_out=eu, status=st)
        else:
            call(b, "dsge_backward_direct_batched", A=Af, B=Bf, D=Df, batch=flat, n=n, k=k, T_out=T, R_out=R)
            st = st * 0  # (this solver reports nothing)
    acc = _or_over_segments(b, st, nb, S)
    return T.reshape(nb, S, n, n), R.reshape(nb, S, n, k), acc


def solve_kalman_logp_segments(b, name, A, B, C, D, Q, Z, y, seg_start, *, solver, tol, max_iter, n_lead_hint, options, **filter_kw):
    """``_solve_segments``, then the filter above.  Returns its dict plus T and R; a draw whose solve fails in any segment gets -inf
    and the OR of the bits."""
    T, R, acc = _solve_segments(b, name, A, B, C, D, Q, Z, y, seg_start, solver, tol, max_iter, n_lead_hint, options)
    res = kalman_logp_segments(b, name, T, R, Q, Z, y, seg_start, status=acc, options=options, **filter_kw)
    res.update(T=T, R=R)
    return res


def solve_kalman_smoother_segments(b, name, A, B, C, D, Q, Z, y, seg_start, *, solver, tol, max_iter, n_lead_hint, options, **smoother_kw):
    """``_solve_segments``, then the smoother across breaks.  Returns its dict plus T and R; a draw whose solve fails in any segment
    has NaN in every output and the OR of the bits."""
    T, R, acc = _solve_segments(b, name, A, B, C, D, Q, Z, y, seg_start, solver, tol, max_iter, n_lead_hint, options)
    res = kalman_smoother_segments(b, name, T, R, Q, Z, y, seg_start, status=acc, options=options, **smoother_kw)
    res.update(T=T, R=R)
    return res


SEGMENT_GRADIENT_OUTPUTS = ("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar", "a0_bar", "P0_bar")
MAX_N_ADJOINT = 56  # dsge_selection_adjoints_batched, dsge_policy_adjoints_batched


def segment_gradient_scratch_bytes_per_draw(m, T_len, n_seg):
    """What ``scratch_limit_bytes`` of the gradient across breaks counts per draw: ``2 T_len m^2 + 2 T_len m`` doubles of the stored
    forward pass and ``2 n_seg m^2`` of the accumulators of ``T_bar`` and of the cotangent of ``sym(R Q R')``."""
    return 8 * (2 * T_len * m * m + 2 * T_len * m + 2 * n_seg * m * m)


def kalman_logp_segments_grad(b, name, T, R, Q, Z, y, seg_start, *, Hdiag, d, a0, P0, shift, q_mode, status, jitter, missing_fill,
                              scratch_limit_bytes, options, outputs=SEGMENT_GRADIENT_OUTPUTS, out=None):
    """``dsge_kalman_logp_segments_grad_batched``: the inputs of ``kalman_logp_segments``.  ``outputs``: which of
    ``SEGMENT_GRADIENT_OUTPUTS`` are computed (logp always is; "Q_bar" is accepted for "q_bar"); ``out``: buffers to reuse.  The
    cotangent of the shock covariance is returned as ``q_bar`` (batch, S, k) for a diagonal layout and as ``Q_bar`` (batch, S, k, k)
    for a full one, per draw also when the covariance is shared."""
    a, _seg = _segment_inputs(b, name, T, R, Q, Z, y, seg_start, Hdiag, d, a0, P0, shift, q_mode)
    nb, S, m, k, p = a["batch"], a["n_seg"], a["m"], a["k"], a["p"]
    if m > _lib.MAX_N or p > _lib.MAX_P:
        raise ValueError(f"{name}: m = {m}, p = {p}; the gradient takes at most {_lib.MAX_N} variables and {_lib.MAX_P} series")
    full = a["q_mode"] in (_lib.Q_FULL_SHARED, _lib.Q_FULL_BATCHED)
    qkey = "Q_bar" if full else "q_bar"
    outputs = tuple("q_bar" if key == "Q_bar" else key for key in outputs)
    if not set(outputs) <= set(SEGMENT_GRADIENT_OUTPUTS):
        raise ValueError(f"outputs must be among {SEGMENT_GRADIENT_OUTPUTS}; got {outputs}")
    limit = 0 if scratch_limit_bytes is None else int(scratch_limit_bytes)
    if limit < 0:
        raise ValueError("scratch_limit_bytes must be >= 0")
    st = check_status(b.status_io(status, nb), nb)
    out = dict(out or {})
    if "Q_bar" in out:
        out["q_bar"] = out.pop("Q_bar")
    shapes = dict(T_bar=(nb, S, m, m), R_bar=(nb, S, m, k), q_bar=(nb, S, k, k) if full else (nb, S, k), Z_bar=(nb, S, p, m),
                  d_bar=(nb, S, p), h_bar=(nb, S, p), shift_bar=(nb, S, m), a0_bar=(nb, m), P0_bar=(nb, m, m))
    res = {key: _out(b, out.get(key), shape) if key in outputs or out.get(key) is not None else None for key, shape in shapes.items()}
    logp = _out(b, out.get("logp"), (nb,))
    with _lib.options_scope(options):  # (the filter conventions: _lib.filter_conventions)
        call(b, "dsge_kalman_logp_segments_grad_batched", **a, jitter=jitter, missing_fill=missing_fill, scratch_limit_bytes=limit,
             logp_out=logp, T_bar=res["T_bar"], R_bar=res["R_bar"], Q_bar=res["q_bar"], Z_bar=res["Z_bar"], d_bar=res["d_bar"],
             h_bar=res["h_bar"], shift_bar=res["shift_bar"], a0_bar=res["a0_bar"], P0_bar=res["P0_bar"], status_io=st)
    res[qkey] = res.pop("q_bar")
    res.update(logp=logp, status=st)
    return res


def solve_kalman_logp_segments_grad(b, name, A, B, C, D, Q, Z, y, seg_start, *, solver, tol, max_iter, n_lead_hint, options,
                                    **grad_kw):
    """``_solve_segments``, the gradient across breaks, then the pullbacks of R = -(C T + B)^-1 D and of the policy function on the
    flattened batch (``dsge_selection_adjoints_batched``, ``dsge_policy_adjoints_batched``, the cotangents of T summed between
    them).  Returns the gradient's dict plus ``A_bar``, ``B_bar``, ``C_bar`` (batch, S, n, n), ``D_bar`` (batch, S, n, k), ``T`` and
    ``R``.  A draw whose solve or adjoint fails in any segment gets -inf, the OR of the bits and zero cotangents."""
    if solver == "backward_direct":
        raise ValueError(f"{name}: backward_direct has no adjoint entry; the solvers are cycle_reduction and gensys")
    Ash = () if A is None else tuple(b.inp(A).shape)
    if len(Ash) == 4 and Ash[2] > MAX_N_ADJOINT:
        raise ValueError(f"{name}: n = {Ash[2]}, the adjoint entries take at most {MAX_N_ADJOINT} variables")
    T, R, acc = _solve_segments(b, name, A, B, C, D, Q, Z, y, seg_start, solver, tol, max_iter, n_lead_hint, options)
    grad_kw["outputs"] = tuple(dict.fromkeys((*grad_kw.get("outputs", SEGMENT_GRADIENT_OUTPUTS), "T_bar", "R_bar")))
    res = kalman_logp_segments_grad(b, name, T, R, Q, Z, y, seg_start, status=acc, options=options, **grad_kw)
    nb, S, n, _ = T.shape
    k, flat = R.shape[3], nb * S
    Bf, Cf = (b.inp(x).reshape(flat, n, n) for x in (B, C))
    Tf, Rf = T.reshape(flat, n, n), R.reshape(flat, n, k)
    Bs, Cs, Ts = (b.empty((flat, n, n)) for _ in range(3))
    Db = b.empty((flat, n, k))
    call(b, "dsge_selection_adjoints_batched", B=Bf, C=Cf, T=Tf, R=Rf, R_bar=res["R_bar"].reshape(flat, n, k), batch=flat, n=n, k=k,
         B_bar=Bs, C_bar=Cs, D_bar=Db, T_bar=Ts)
    Tsum = Ts + res["T_bar"].reshape(flat, n, n)
    Ab, Bb, Cb = (b.empty((flat, n, n)) for _ in range(3))
    ast = b.empty((flat,), "int32")
    call(b, "dsge_policy_adjoints_batched", B=Bf, C=Cf, T=Tf, T_bar=b.inp(Tsum if b.host else Tsum.contiguous()), batch=flat, n=n,
         A_bar=Ab, B_bar=Bb, C_bar=Cb, status=ast)
    Bb, Cb = Bb + Bs, Cb + Cs
    # a failed draw: the OR of the bits, -inf, zeros -- with array operations of the backend (no host round trip on the device)
    xp = b.xp
    # (the adjoint of a draw the filter skipped ran on zeros: its word says nothing, the draw keeps the filter's)
    st = xp.where(res["status"] != 0, res["status"], _or_over_segments(b, ast, nb, S))
    res["status"] = st
    bad = st != 0
    res["logp"][...] = xp.where(bad, xp.full_like(res["logp"], -np.inf), res["logp"])
    res.update(A_bar=Ab.reshape(nb, S, n, n), B_bar=Bb.reshape(nb, S, n, n), C_bar=Cb.reshape(nb, S, n, n),
               D_bar=Db.reshape(nb, S, n, k), T=T, R=R)
    for key, val in res.items():
        if key.endswith("_bar") and val is not None:
            val[...] = xp.where(bad.reshape((nb,) + (1,) * (val.ndim - 1)), xp.zeros_like(val), val)
    return res


def shock_groups(groups, k):
    """``groups`` (None, or a sequence of sequences of shock indices that partitions 0 .. k-1) -> (group_of_shock int32 (k,), g)."""
    if groups is None:
        return np.arange(k, dtype=np.int32), k
    of = np.full(k, -1, dtype=np.int32)
    try:
        members = [[int(j) for j in grp] for grp in groups]
    except TypeError:
        raise ValueError("groups must be a sequence of sequences of shock indices") from None
    for c, grp in enumerate(members):
        if not grp:
            raise ValueError(f"groups[{c}] is empty")
        for j in grp:
            if not 0 <= j < k:
                raise ValueError(f"groups[{c}] holds {j}: shock indices are 0 .. {k - 1}")
            if of[j] >= 0:
                raise ValueError(f"shock {j} is in groups[{of[j]}] and in groups[{c}]")
            of[j] = c
    if (of < 0).any():
        raise ValueError(f"groups must partition 0 .. {k - 1}: shocks {np.flatnonzero(of < 0).tolist()} are in no group")
    return of, len(members)


def shock_decomposition(b, name, T, R, states, shocks, *, groups, variables, Z, remainder, status, out=None):
    """``states`` / ``shocks``: (batch, T_len, m) / (batch, T_len, k) of the smoother or (batch, n_paths, T_len, .) of the
    simulation smoother; the outputs have the same number of leading axes."""
    T, R, nb, m, k = _TR(b, T, R, name)
    states, shocks = b.inp(states), b.inp(shocks)
    if states.ndim not in (3, 4) or shocks.ndim != states.ndim:
        raise ValueError(f"states and shocks must both be (batch, T_len, .) or (batch, n_paths, T_len, .); got {tuple(states.shape)}, "
                         f"{tuple(shocks.shape)}")
    lead = tuple(states.shape[:-1])
    if lead[0] != nb or states.shape[-1] != m or tuple(shocks.shape) != (*lead, k):
        raise ValueError(f"states must be {(nb, '...', m)} and shocks {(nb, '...', k)} with the same leading axes; got "
                         f"{tuple(states.shape)}, {tuple(shocks.shape)}")
    n_paths, T_len = (1, lead[1]) if len(lead) == 2 else lead[1:]
    if T_len < 1:
        raise ValueError("states holds no period")
    grp, g = shock_groups(groups, k)
    if variables is None:
        var = np.arange(m, dtype=np.int32)
    else:
        var = np.asarray(list(variables), dtype=np.int64).reshape(-1)
        if ((var < 0) | (var >= m)).any():
            raise ValueError(f"variables must be within 0 .. {m - 1}; got {var.tolist()}")
        if len(np.unique(var)) != len(var):
            raise ValueError(f"variables holds a variable twice: {var.tolist()}")
        var = np.ascontiguousarray(var, dtype=np.int32)
    n_out, p, zb = len(var), 0, 0
    if Z is not None:
        Z = b.inp(Z)
        if Z.ndim not in (2, 3) or Z.shape[-1] != m or Z.shape[-2] < 1:
            raise ValueError(f"Z must be (p, {m}) or (batch, p, {m}); got {tuple(Z.shape)}")
        p = Z.shape[-2]
        zb = shared_or_batched(Z, nb, (p, m), "Z")
    if n_out == 0 and p == 0:
        raise ValueError("nothing requested: no variables and no Z")
    st = check_status(b.inp(status, "int32"), nb)
    C = g + 1 + bool(remainder)
    out = out or {}
    res = dict(contributions=_out(b, out.get("contributions"), (*lead, n_out, C)) if n_out else None,
               observed=_out(b, out.get("observed"), (*lead, p, C)) if p else None,
               components=[*range(g), "initial"] + (["remainder"] if remainder else []))
    call(b, "dsge_shock_decomposition_batched", T=T, R=R, eps=shocks, x=states, group_of_shock=grp.ctypes.data, n_groups=g,
         var_idx=var.ctypes.data, n_out=n_out, Z=Z, z_batched=zb, status=st, batch=nb, m=m, k=k, p=p, n_paths=n_paths, T_len=T_len,
         remainder=bool(remainder), contrib_out=res["contributions"], obs_out=res["observed"])
    return res


def condition_pattern(conditions, nb, n_paths, p, n_steps):
    """``conditions``: (h_c, p), (batch, h_c, p) or (batch, n_paths, h_c, p), NaN = free, the same NaN pattern for every draw and
    path -- or the triple ``(cond_t, cond_j, values)`` with ``values`` (n_cond,), (batch, n_cond) or (batch, n_paths, n_cond), which
    needs no look at the values (device tensors: no synchronisation).  -> (cond_t int32, cond_j int32, values (..., n_cond))."""
    if isinstance(conditions, tuple):
        if len(conditions) != 3:
            raise ValueError("conditions as a tuple must be (cond_t, cond_j, values)")
        ct, cj = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in conditions[:2])
        vals = conditions[2]
        if len(ct) != len(cj) or vals.shape[-1] != len(ct) or vals.ndim not in (1, 2, 3):
            raise ValueError(f"conditions: cond_t, cond_j and the last axis of values must have one length; got {len(ct)}, {len(cj)}, "
                             f"{tuple(vals.shape)}")
        return ct, cj, vals
    c = conditions
    if c.ndim not in (2, 3, 4) or c.shape[-1] != p:
        raise ValueError(f"conditions must be (h_c, {p}), (batch, h_c, {p}) or (batch, n_paths, h_c, {p}); got {tuple(c.shape)}")
    if tuple(c.shape[:-2]) not in ((), (nb,), (nb, n_paths)):
        raise ValueError(f"conditions: leading axes must be (), ({nb},) or ({nb}, {n_paths}); got {tuple(c.shape[:-2])}")
    h_c = c.shape[-2]
    if h_c > n_steps:
        raise ValueError(f"conditions cover {h_c} periods, n_steps is {n_steps}")
    host = np.asarray(c.cpu() if hasattr(c, "cpu") else c)
    free = np.isnan(host).reshape(-1, h_c, p)
    if (free != free[0]).any():
        raise ValueError("conditions: the NaN pattern (which series is conditioned in which period) must be the same for every draw and path")
    ct, cj = (np.ascontiguousarray(v, dtype=np.int32) for v in np.nonzero(~free[0]))  # row-major: ascending in (t, j)
    return ct, cj, c[..., ct.tolist(), cj.tolist()]


def conditional_forecast(b, name, T, R, Q, x0, conditions, n_steps, *, Z, d, eps, n_paths, free_shocks, q_mode, status, rank_tol,
                         out=None):
    T, R, nb, m, k = _TR(b, T, R, name)
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    if Z is None:
        raise ValueError(f"{name}: Z is required (the conditions are on d + Z x)")
    Z = b.inp(Z)
    if Z.ndim not in (2, 3) or Z.shape[-1] != m or Z.shape[-2] < 1:
        raise ValueError(f"Z must be (p, {m}) or (batch, p, {m}); got {tuple(Z.shape)}")
    p = Z.shape[-2]
    obs = obs_args(b, Z, d, None, nb, p, m)
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    # the number of paths: the shocks say it, else n_paths, else a per-path x0 or conditions, else one
    eps, eb, n_shock = b.inp(eps), 0, 0
    x0 = b.inp(x0)
    if x0.ndim not in (1, 2, 3) or x0.shape[-1] != m:
        raise ValueError(f"x0 must be ({m},), (batch, {m}) or (batch | 1, n_paths | 1, {m}); got {tuple(x0.shape)}")
    guess = [eps.shape[-3]] if eps is not None and eps.ndim in (3, 4) else []
    guess += [int(n_paths)] if n_paths is not None else []
    guess += [x0.shape[1]] if x0.ndim == 3 and x0.shape[1] != 1 else []
    guess += [conditions.shape[1]] if not isinstance(conditions, tuple) and conditions.ndim == 4 else []
    guess += [conditions[2].shape[1]] if isinstance(conditions, tuple) and len(conditions) == 3 and conditions[2].ndim == 3 else []
    n_paths = guess[0] if guess else 1
    if n_paths < 1 or any(g != n_paths for g in guess):
        raise ValueError(f"n_paths must be >= 1 and eps, n_paths, x0 and conditions must agree on it; got {guess}")
    if eps is not None:
        if eps.ndim not in (3, 4) or eps.shape[-1] != k:
            raise ValueError(f"eps must be (n_paths, n_shock_steps, {k}) or (batch, n_paths, n_shock_steps, {k}); got {tuple(eps.shape)}")
        n_shock = eps.shape[-2]
        eb = shared_or_batched(eps, nb, (n_paths, n_shock, k), "eps")
        if n_shock > n_steps:
            raise ValueError(f"n_steps = {n_steps} is less than the {n_shock} shock steps of eps")
    if x0.ndim == 3:
        if x0.shape[0] not in (1, nb) or x0.shape[1] not in (1, n_paths):
            raise ValueError(f"x0 must be (batch | 1, n_paths | 1, {m}); got {tuple(x0.shape)}")
        xb, xpth = int(x0.shape[0] == nb), int(x0.shape[1] == n_paths)
    else:
        xb, xpth = (shared_or_batched(x0, nb, (m,), "x0"), 0)
    ct, cj, vals = condition_pattern(conditions if isinstance(conditions, tuple) else (b.inp(conditions) if not b.host else
                                     np.asarray(conditions, dtype=np.float64)), nb, n_paths, p, n_steps)
    n_cond = len(ct)
    vals = b.inp(vals if b.host else vals.contiguous())
    lead = tuple(vals.shape[:-1])
    if lead not in ((), (nb,), (nb, n_paths)):
        raise ValueError(f"the values of the conditions must be (n_cond,), ({nb}, n_cond) or ({nb}, {n_paths}, n_cond); got {tuple(vals.shape)}")
    cvb, cvp = int(len(lead) >= 1), int(len(lead) == 2)
    if free_shocks is None:
        free = None
    else:
        fs = np.asarray(list(free_shocks))
        if fs.dtype == bool:
            if fs.shape != (k,):
                raise ValueError(f"free_shocks as a mask must have {k} entries")
            free = np.ascontiguousarray(fs, dtype=np.int32)
        else:
            fs = fs.astype(np.int64).reshape(-1)
            if ((fs < 0) | (fs >= k)).any():
                raise ValueError(f"free_shocks must be within 0 .. {k - 1}; got {fs.tolist()}")
            free = np.zeros(k, dtype=np.int32)
            free[fs] = 1
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    res = dict(x=_out(b, out.get("x"), (nb, n_paths, n_steps, m)), shocks=_out(b, out.get("shocks"), (nb, n_paths, n_steps, k)),
               observed=_out(b, out.get("observed"), (nb, n_paths, n_steps, p)), status=st)
    call(b, "dsge_conditional_forecast_batched", T=T, R=R, Q=Q, q_mode=code, Z=obs["Z"], z_batched=obs["z_batched"], d=obs["d"],
         d_batched=obs["d_batched"], x0=x0, x0_batched=xb, x0_paths=xpth, eps=eps, eps_batched=eb,
         cond_t=ct.ctypes.data if n_cond else None, cond_j=cj.ctypes.data if n_cond else None, n_cond=n_cond,
         cond_val=vals if n_cond else None, cv_batched=cvb, cv_paths=cvp, free_shock=None if free is None else free.ctypes.data,
         status_io=st, batch=nb, m=m, k=k, p=p, n_paths=n_paths, n_steps=n_steps, n_shock_steps=n_shock,
         rank_tol=0.0 if rank_tol is None else float(rank_tol), x_out=res["x"], eps_out=res["shocks"], obs_out=res["observed"])
    return res


def spectral_freqs(n_grid):
    """The grid ``w_n = 2 pi n / N``, ``n = 0 .. N/2`` (host float64); ``N`` even and within 4 .. 4096."""
    n_grid = int(n_grid)
    if n_grid < 4 or n_grid > 4096 or n_grid % 2:
        raise ValueError(f"n_grid must be even and within 4 .. 4096; got {n_grid}")
    return 2.0 * np.pi * np.arange(n_grid // 2 + 1) / n_grid


def hp_gain(n_grid, lam=1600.0):
    """The squared gain of the Hodrick-Prescott cyclical filter on the grid of ``spectral_moments``:
    ``(4 lam (1 - cos w)^2 / (1 + 4 lam (1 - cos w)^2))^2``, exactly 0 at ``w = 0``."""
    c = 4.0 * float(lam) * (1.0 - np.cos(spectral_freqs(n_grid))) ** 2
    g = (c / (1.0 + c)) ** 2
    g[0] = 0.0
    return g


def bandpass_gain(n_grid, low=6, high=32):
    """The squared gain of the ideal band-pass filter that keeps the periods ``low .. high``: 1 where
    ``2 pi / high <= w <= 2 pi / low``, else 0."""
    if not 0 < low <= high:
        raise ValueError(f"bandpass_gain needs 0 < low <= high; got {low}, {high}")
    n = np.arange(len(spectral_freqs(n_grid)))
    # w_n = 2 pi n / N within [2 pi / high, 2 pi / low], decided without rounding the grid: an edge on a grid point is in the band
    return ((n * high >= n_grid) & (n * low <= n_grid)).astype(np.float64)


def spectral_moments(b, name, T, R, Q, *, n_grid, n_lags, Z, Hdiag, gain, correlation, spectrum, acov=True, q_mode, status, rank_tol,
                     scratch_limit_bytes, out=None):
    T, R, nb, m, k = _TR(b, T, R, name)
    Q = b.inp(Q)
    code = q_layout(Q.shape, q_mode, nb, k)
    freqs = spectral_freqs(n_grid)
    n_grid, nf, n_lags = int(n_grid), len(freqs), int(n_lags)
    if n_lags < 0 or n_lags > n_grid // 2:
        raise ValueError(f"n_lags must be within 0 .. n_grid / 2 = {n_grid // 2}; got {n_lags}")
    if Z is None:
        if Hdiag is not None:
            raise ValueError(f"{name}: Hdiag (measurement noise) needs Z")
        obs, p, dim = dict(Z=None, z_batched=0, Hdiag=None, h_batched=0), 0, m
    else:
        Z = b.inp(Z)
        if Z.ndim not in (2, 3) or Z.shape[-1] != m or Z.shape[-2] < 1:
            raise ValueError(f"Z must be (p, {m}) or (batch, p, {m}); got {tuple(Z.shape)}")
        p = dim = Z.shape[-2]
        obs = obs_args(b, Z, None, Hdiag, nb, p, m)
        obs = {key: obs[key] for key in ("Z", "z_batched", "Hdiag", "h_batched")}
    gain = b.inp(gain)
    if gain is not None:
        _is(gain, (nf,), "gain", f"({nf},) = (n_grid / 2 + 1,)")
    if not (acov or spectrum):
        raise ValueError(f"{name}: nothing to compute (acov and spectrum are both off)")
    limit = 0 if scratch_limit_bytes is None else int(scratch_limit_bytes)
    if limit < 0:
        raise ValueError("scratch_limit_bytes must be >= 0")
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    res = dict(acov=_out(b, out.get("acov"), (nb, n_lags + 1, dim, dim)) if acov else None, freqs=freqs, status=st)
    spec = _out(b, out.get("spectrum"), (nb, nf, dim, dim), "complex128") if spectrum else None
    if spectrum:
        res["spectrum"] = spec
    call(b, "dsge_spectral_moments_batched", T=T, R=R, Q=Q, q_mode=code, **obs, gain=gain, batch=nb, m=m, k=k, p=p, n_grid=n_grid,
         n_lags=n_lags, correlation=int(bool(correlation)), rank_tol=0.0 if rank_tol is None else float(rank_tol),
         scratch_limit_bytes=limit, acov_out=res["acov"], spectrum_out=spec, status_io=st)
    return res


# ---- anticipated shocks ----------------------------------------------------------------------------------------------------------
ANT_MODES = {"perfect_foresight": _lib.ANT_PERFECT_FORESIGHT, "news": _lib.ANT_NEWS}
ANT_OUTPUTS = ("x", "w", "observed", "G")


def expected_shocks_from_news(nu):
    """Arrivals of news -> expected shocks (host arrays).  ``nu[..., t, j, :]`` is what is learnt at ``t`` about the shock of
    ``t + j`` (``j = 0 .. n_lead``); the result ``e[..., t, j, :] = E_t eps_{t+j} = sum_{i = 0 .. min(t, n_lead - j)} nu[..., t - i, j + i, :]``
    is what ``anticipated_paths`` takes in news mode."""
    nu = np.asarray(nu, dtype=np.float64)
    if nu.ndim < 3:
        raise ValueError(f"nu must be (..., n_shock_steps, n_lead + 1, k); got {nu.shape}")
    steps, leads = nu.shape[-3], nu.shape[-2]
    e = np.zeros_like(nu)
    for i in range(min(steps, leads)):  # what was learnt i periods earlier
        e[..., i:, :leads - i, :] += nu[..., :steps - i, i:, :]
    return e


def _ant_x0(b, x0, nb, n_paths, n):
    """x0: (n,) shared by all, (n_paths, n) per path as ``simulate`` takes it, or (batch | 1, n_paths | 1, n) -> (x0, x0_batched,
    x0_paths)."""
    x0 = b.inp(x0)
    xb = xpth = 0
    if x0 is not None:
        shape = tuple(x0.shape)
        if shape == (n,):
            pass
        elif shape == (n_paths, n):
            xpth = 1
        elif len(shape) == 3 and shape[0] in (1, nb) and shape[1] in (1, n_paths) and shape[2] == n:
            xb, xpth = int(shape[0] == nb), int(shape[1] == n_paths)
        else:
            raise ValueError(f"x0 must be ({n},), ({n_paths}, {n}) or (batch | 1, n_paths | 1, {n}); got {shape}")
    return x0, xb, xpth


def _ant_obs(b, name, Z, d, outputs, nb, n):
    """The observation equation of the output "observed" -> (dict(Z, z_batched, d, d_batched), p)."""
    if Z is None:
        if d is not None or "observed" in outputs:
            raise ValueError(f"{name}: d and the output 'observed' need Z")
        return dict(Z=None, z_batched=0, d=None, d_batched=0), 0
    Z = b.inp(Z)
    if Z.ndim not in (2, 3) or Z.shape[-1] != n or Z.shape[-2] < 1:
        raise ValueError(f"Z must be (p, {n}) or (batch, p, {n}); got {tuple(Z.shape)}")
    p = Z.shape[-2]
    if p > _lib.MAX_P:
        raise ValueError(f"{name}: p = {p}, at most {_lib.MAX_P} observed series")
    obs = obs_args(b, Z, d, None, nb, p, n)
    return {key: obs[key] for key in ("Z", "z_batched", "d", "d_batched")}, p


def anticipated_paths(b, name, B, C, T, R, eps, *, n_steps, mode, x0, Z, d, status, rank_tol, outputs, out=None):
    T, R, nb, n, k = _TR(b, T, R, name)
    if n > _lib.MAX_N:
        raise ValueError(f"{name}: n = {n}, at most {_lib.MAX_N} variables (models of 65 .. {_lib.MAX_N_BIG} are out of scope here)")
    B, C = _nd(b.inp(B), 3), _nd(b.inp(C), 3)
    if tuple(B.shape) != (nb, n, n) or tuple(C.shape) != (nb, n, n):
        raise ValueError(f"B and C must be {(nb, n, n)} like T; got {tuple(B.shape)}, {tuple(C.shape)}")
    if mode not in ANT_MODES:
        raise ValueError(f"mode must be one of {sorted(ANT_MODES)}; got {mode!r}")
    news = int(mode == "news")
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in ANT_OUTPUTS for o in outputs):
        raise ValueError(f"outputs must name at least one of {ANT_OUTPUTS}; got {outputs}")
    eps = b.inp(eps)
    tail = "n_shock_steps, n_lead + 1" if news else "n_shock_steps"
    if eps.ndim not in (3 + news, 4 + news) or eps.shape[-1] != k:
        raise ValueError(f"eps must be (n_paths, {tail}, {k}) or (batch, n_paths, {tail}, {k}) in mode {mode!r}; got {tuple(eps.shape)}")
    n_paths, n_shock = eps.shape[-3 - news], eps.shape[-2 - news]
    n_lead = eps.shape[-2] - 1 if news else 0
    if n_lead < 0 or n_lead > _lib.ANT_MAX_LEAD:
        raise ValueError(f"{name}: n_lead = {n_lead} is outside 0 .. {_lib.ANT_MAX_LEAD}")
    eb = shared_or_batched(eps, nb, tuple(eps.shape[-3 - news:]), "eps")
    n_steps = n_shock if n_steps is None else int(n_steps)
    if n_steps < 0 or (news and n_steps < n_shock):
        raise ValueError(f"n_steps = {n_steps}: news needs at least the {n_shock} shock steps of eps, perfect foresight at least 0")
    x0, xb, xpth = _ant_x0(b, x0, nb, n_paths, n)
    obs, p = _ant_obs(b, name, Z, d, outputs, nb, n)
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    shapes = dict(x=(nb, n_paths, n_steps, n), w=(nb, n_paths, n_steps, n), observed=(nb, n_paths, n_steps, p), G=(nb, n, n))
    res = {key: _out(b, out.get(key), shapes[key]) for key in ANT_OUTPUTS if key in outputs}
    res["status"] = st
    call(b, "dsge_anticipated_paths_batched", B=B, C=C, T=T, R=R, eps=eps if n_shock > 0 else None, eps_batched=eb,
         mode=ANT_MODES[mode], n_lead=n_lead, x0=x0, x0_batched=xb, x0_paths=xpth, **obs, status_io=st, batch=nb, n=n, k=k, p=p,
         n_paths=n_paths, n_steps=n_steps, n_shock_steps=n_shock, rank_tol=0.0 if rank_tol is None else float(rank_tol),
         x_out=res.get("x"), w_out=res.get("w"), obs_out=res.get("observed"), G_out=res.get("G"))
    return res


# ---- occasionally binding bound ----------------------------------------------------------------------------------------------------
OBC_OUTPUTS = ("x", "w", "observed", "nu", "gap", "Mz", "path_status", "iters")


def constrained_paths(b, name, B, C, T, R, eps, c, bound, shock, horizon, *, n_steps, x0, Z, d, status, rank_tol, max_iter, outputs,
                      out=None):
    T, R, nb, n, k = _TR(b, T, R, name)
    if n > _lib.MAX_N:
        raise ValueError(f"{name}: n = {n}, at most {_lib.MAX_N} variables (models of 65 .. {_lib.MAX_N_BIG} are out of scope here)")
    B, C = _nd(b.inp(B), 3), _nd(b.inp(C), 3)
    if tuple(B.shape) != (nb, n, n) or tuple(C.shape) != (nb, n, n):
        raise ValueError(f"B and C must be {(nb, n, n)} like T; got {tuple(B.shape)}, {tuple(C.shape)}")
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in OBC_OUTPUTS for o in outputs):
        raise ValueError(f"outputs must name at least one of {OBC_OUTPUTS}; got {outputs}")
    eps = b.inp(eps)
    if eps.ndim not in (3, 4) or eps.shape[-1] != k:
        raise ValueError(f"eps must be (n_paths, n_shock_steps, {k}) or (batch, n_paths, n_shock_steps, {k}); got {tuple(eps.shape)}")
    n_paths, n_shock = eps.shape[-3], eps.shape[-2]
    eb = shared_or_batched(eps, nb, tuple(eps.shape[-3:]), "eps")
    n_steps = n_shock if n_steps is None else int(n_steps)
    shock, horizon = int(shock), int(horizon)
    if not 0 <= shock < k:
        raise ValueError(f"{name}: shock = {shock} is outside 0 .. {k - 1}")
    if not 1 <= horizon <= _lib.OBC_MAX_HORIZON:
        raise ValueError(f"{name}: horizon = {horizon} is outside 1 .. {_lib.OBC_MAX_HORIZON}")
    if n_steps < 0 or (n_steps > 0 and horizon > n_steps):
        raise ValueError(f"{name}: n_steps = {n_steps} must hold the horizon of {horizon} periods")
    if c is None or bound is None:
        raise ValueError(f"{name}: the constraint row c and the bound are needed")
    c = b.inp(c)
    cb = shared_or_batched(c, nb, (n,), "c", f"({n},) or (batch, {n})")
    if isinstance(bound, (int, float)):
        value, bound = float(bound), b.empty((1,))
        bound[...] = value
    bound = b.inp(bound)
    if tuple(bound.shape) not in ((), (1,), (nb,)):
        raise ValueError(f"bound must be a number, (1,) or (batch,); got {tuple(bound.shape)}")
    bb = int(tuple(bound.shape) == (nb,) and nb > 1)
    x0, xb, xpth = _ant_x0(b, x0, nb, n_paths, n)
    obs, p = _ant_obs(b, name, Z, d, outputs, nb, n)
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    path = (nb, n_paths, n_steps)
    shapes = dict(x=path + (n,), w=path + (n,), observed=path + (p,), nu=(nb, n_paths, horizon), gap=path, Mz=(nb, horizon, horizon),
                  path_status=(nb, n_paths), iters=(nb, n_paths))
    res = {key: _out(b, out.get(key), shapes[key], "int32" if key in ("path_status", "iters") else "float64")
           for key in OBC_OUTPUTS if key in outputs}
    res["status"] = st
    call(b, "dsge_constrained_paths_batched", B=B, C=C, T=T, R=R, eps=eps if n_shock > 0 else None, eps_batched=eb, x0=x0,
         x0_batched=xb, x0_paths=xpth, **obs, c_row=c, c_batched=cb, bound=bound, bound_batched=bb, shock=shock, horizon=horizon,
         max_iter=0 if max_iter is None else int(max_iter), status_io=st, batch=nb, n=n, k=k, p=p, n_paths=n_paths, n_steps=n_steps,
         n_shock_steps=n_shock, rank_tol=0.0 if rank_tol is None else float(rank_tol), x_out=res.get("x"), w_out=res.get("w"),
         obs_out=res.get("observed"), nu_out=res.get("nu"), gap_out=res.get("gap"), Mz_out=res.get("Mz"),
         path_status_out=res.get("path_status"), iters_out=res.get("iters"))
    return res


# ---- stochastic simulation at the bound ----------------------------------------------------------------------------------------------
OBC_SIM_OUTPUTS = ("x", "observed", "gap", "shadow", "plan", "duration", "iters", "Mz", "path_status", "fail_step")


def constrained_simulate(b, name, B, C, T, R, eps, c, bound, shock, horizon, *, n_steps, x0, Z, d, status, rank_tol, max_iter,
                         outputs, out=None):
    T, R, nb, n, k = _TR(b, T, R, name)
    if n > _lib.MAX_N:
        raise ValueError(f"{name}: n = {n}, at most {_lib.MAX_N} variables (models of 65 .. {_lib.MAX_N_BIG} are out of scope here)")
    B, C = _nd(b.inp(B), 3), _nd(b.inp(C), 3)
    if tuple(B.shape) != (nb, n, n) or tuple(C.shape) != (nb, n, n):
        raise ValueError(f"B and C must be {(nb, n, n)} like T; got {tuple(B.shape)}, {tuple(C.shape)}")
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or any(o not in OBC_SIM_OUTPUTS for o in outputs):
        raise ValueError(f"outputs must name at least one of {OBC_SIM_OUTPUTS}; got {outputs}")
    eps = b.inp(eps)
    if eps.ndim not in (3, 4) or eps.shape[-1] != k:
        raise ValueError(f"eps must be (n_paths, n_shock_steps, {k}) or (batch, n_paths, n_shock_steps, {k}); got {tuple(eps.shape)}")
    n_paths, n_shock = eps.shape[-3], eps.shape[-2]
    eb = shared_or_batched(eps, nb, tuple(eps.shape[-3:]), "eps")
    n_steps = n_shock if n_steps is None else int(n_steps)
    shock, horizon = int(shock), int(horizon)
    if not 0 <= shock < k:
        raise ValueError(f"{name}: shock = {shock} is outside 0 .. {k - 1}")
    if not 1 <= horizon <= _lib.OBC_MAX_HORIZON:
        raise ValueError(f"{name}: horizon = {horizon} is outside 1 .. {_lib.OBC_MAX_HORIZON}")
    if n_steps < 0 or n_shock > n_steps:
        raise ValueError(f"{name}: n_steps = {n_steps} must be at least the {n_shock} shock steps of eps")
    if c is None or bound is None:
        raise ValueError(f"{name}: the constraint row c and the bound are needed")
    c = b.inp(c)
    cb = shared_or_batched(c, nb, (n,), "c", f"({n},) or (batch, {n})")
    if isinstance(bound, (int, float)):
        value, bound = float(bound), b.empty((1,))
        bound[...] = value
    bound = b.inp(bound)
    if tuple(bound.shape) not in ((), (1,), (nb,)):
        raise ValueError(f"bound must be a number, (1,) or (batch,); got {tuple(bound.shape)}")
    bb = int(tuple(bound.shape) == (nb,) and nb > 1)
    x0, xb, xpth = _ant_x0(b, x0, nb, n_paths, n)
    obs, p = _ant_obs(b, name, Z, d, outputs, nb, n)
    st = check_status(b.status_io(status, nb), nb)
    out = out or {}
    path = (nb, n_paths, n_steps)
    shapes = dict(x=path + (n,), observed=path + (p,), gap=path, shadow=path, plan=path + (horizon,), duration=path, iters=path,
                  Mz=(nb, horizon, horizon), path_status=(nb, n_paths), fail_step=(nb, n_paths))
    ints = ("duration", "iters", "path_status", "fail_step")
    res = {key: _out(b, out.get(key), shapes[key], "int32" if key in ints else "float64") for key in OBC_SIM_OUTPUTS if key in outputs}
    res["status"] = st
    call(b, "dsge_constrained_simulate_batched", B=B, C=C, T=T, R=R, eps=eps if n_shock > 0 else None, eps_batched=eb, x0=x0,
         x0_batched=xb, x0_paths=xpth, **obs, c_row=c, c_batched=cb, bound=bound, bound_batched=bb, shock=shock, horizon=horizon,
         max_iter=0 if max_iter is None else int(max_iter), status_io=st, batch=nb, n=n, k=k, p=p, n_paths=n_paths, n_steps=n_steps,
         n_shock_steps=n_shock, rank_tol=0.0 if rank_tol is None else float(rank_tol), x_out=res.get("x"), obs_out=res.get("observed"),
         gap_out=res.get("gap"), shadow_out=res.get("shadow"), plan_out=res.get("plan"), duration_out=res.get("duration"),
         iters_out=res.get("iters"), Mz_out=res.get("Mz"), path_status_out=res.get("path_status"), fail_step_out=res.get("fail_step"))
    return res


# ---- second-order dynamics: the pruned recursion on the solution of ``second_order_logp`` ----------------------------------------
SOLUTION =("T", "R", "g_yy", "g_yu", "g_uu", "g_ss", "S")


def bind_solution(fname, args, kwargs, rest):
    """The calling convention of the second-order dynamics: ``T, R, g_yy, g_yu, g_uu, g_ss, S`` or, in their place, ONE dict that
    holds them (what ``second_order_logp_batched(..., return_solution=True)`` returns), followed by ``rest`` = ((name, default), ...)
    by position or by name.  -> (the solution dict, the dict of the rest)."""
    packed = bool(args) and isinstance(args[0], dict)
    names = (("solution",) if packed else SOLUTION) + tuple(name for name, _ in rest)
    if len(args) > len(names):
        raise TypeError(f"{fname} takes at most {len(names)} positional arguments; got {len(args)}")
    bound = dict(zip(names, args))
    for key, value in kwargs.items():
        if key not in names or key in bound:
            raise TypeError(f"{fname}: {'unknown' if key not in names else 'repeated'} argument {key!r}")
        bound[key] = value
    sol = bound.pop("solution") if packed else {key: bound.pop(key) for key in SOLUTION if key in bound}
    missing = [key for key in SOLUTION if key not in sol]
    if missing:
        raise TypeError(f"{fname}: the second-order solution lacks {missing}")
    return sol, {name: bound.get(name, default) for name, default in rest}


def _pruned_solution(b, sol):
    """The validated coefficients as named arguments, and (batch, n, k)."""
    T, R = _nd(b.inp(sol["T"]), 3), _nd(b.inp(sol["R"]), 3)
    nb, n, n2 = T.shape
    if n != n2 or tuple(R.shape[:2]) != (nb, n) or R.shape[2] < 1:
        raise ValueError(f"T must be (batch, n, n) and R (batch, n, k); got {tuple(T.shape)}, {tuple(R.shape)}")
    k = R.shape[2]
    g_yy = _nd(b.inp(sol["g_yy"]), 4)
    s = g_yy.shape[-1]
    S = np.asarray(sol["S"])  # (a host index list for both backends, as in the second-order entry)
    if S.ndim != 1 or len(S) != s or not np.issubdtype(S.dtype, np.integer):
        raise ValueError(f"S must be an index list of length g_yy.shape[-1] = {s}; got shape {S.shape}, dtype {S.dtype}")
    if s < 1 or S[0] < 0 or S[-1] >= n or (np.diff(S) <= 0).any():
        raise ValueError(f"S must be strictly ascending within 0 .. {n - 1}; got {S.tolist()}")
    _is(g_yy, (nb, n, s, s), "g_yy", "(batch, n, s, s)")
    g_yu = _is(b.inp(sol["g_yu"]), (nb, n, s, k), "g_yu", "(batch, n, s, k)")
    g_uu = _is(b.inp(sol["g_uu"]), (nb, n, k, k), "g_uu", "(batch, n, k, k)")
    g_ss = _is(b.inp(sol["g_ss"]), (nb, n), "g_ss", "(batch, n)")
    S = np.ascontiguousarray(S, dtype=np.int32)
    return dict(T=T, R=R, gyy=g_yy, gyu=g_yu, guu=g_uu, gss=g_ss, state_idx=S.ctypes.data, n_state=s, batch=nb, n=n, k=k), S, (nb, n, k)


def _pruned_paths(b, eps, x0, n_steps, nb, n, k):
    """Shocks (may be None: one path without shocks), the initial pair and the step counts as named arguments."""
    n_paths, n_shock, eb = 1, 0, 0
    if eps is not None:
        eps = b.inp(eps)
        if eps.ndim not in (3, 4) or eps.shape[-1] != k:
            raise ValueError(f"eps must be (n_paths, n_shock_steps, {k}) or (batch, n_paths, n_shock_steps, {k}); got {tuple(eps.shape)}")
        n_paths, n_shock = eps.shape[-3], eps.shape[-2]
        eb = shared_or_batched(eps, nb, (n_paths, n_shock, k), "eps")
    n_steps = n_shock if n_steps is None else int(n_steps)
    if n_steps < n_shock:
        raise ValueError(f"n_steps = {n_steps} is less than the {n_shock} shock steps of eps")
    xf0 = xs0 = None
    xb = 0
    if x0 is not None:
        if not isinstance(x0, (tuple, list)) or len(x0) != 2:
            raise ValueError("x0 must be None or a pair (xf0, xs0)")
        xf0, xs0 = b.inp(x0[0]), b.inp(x0[1])
        if tuple(xf0.shape) != tuple(xs0.shape):
            raise ValueError(f"the x0 pair must have one shape; got {tuple(xf0.shape)} and {tuple(xs0.shape)}")
        xb = shared_or_batched(xf0, nb, (n_paths, n), "x0")
    return dict(eps=eps, eps_batched=eb, xf0=xf0, xs0=xs0, x0_batched=xb, n_paths=n_paths, n_steps=n_steps, n_shock_steps=n_shock)


def simulate_pruned(b, sol, eps, *, n_steps, x0, status, parts, out=None):
    a, S, (nb, n, k) = _pruned_solution(b, sol)
    if eps is None:
        raise ValueError("eps is required: (n_paths, n_shock_steps, k) or (batch, n_paths, n_shock_steps, k)")
    a.update(_pruned_paths(b, eps, x0, n_steps, nb, n, k))
    st = check_status(b.inp(status, "int32"), nb)
    out = out or {}
    shape = (nb, a["n_paths"], a["n_steps"], n)
    res = dict(x=_out(b, out.get("x"), shape))
    for key in ("x_f", "x_s"):
        if parts or out.get(key) is not None:
            res[key] = _out(b, out.get(key), shape)
    call(b, "dsge_simulate_pruned_batched", **a, status=st, x_out=res["x"], xf_out=res.get("x_f"), xs_out=res.get("x_s"))
    return res


def girf_pruned(b, sol, *, n_steps, impulses, eps, x0, status, out=None):
    a, S, (nb, n, k) = _pruned_solution(b, sol)
    sb, c = 0, k
    if impulses is not None:
        impulses = b.inp(impulses)
        if impulses.ndim not in (2, 3) or impulses.shape[-2] != k:
            raise ValueError(f"impulses must be ({k}, c) or (batch, {k}, c); got {tuple(impulses.shape)}")
        c = impulses.shape[-1]
        sb = shared_or_batched(impulses, nb, (k, c), "impulses")
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError("n_steps must be >= 0")
    a.update(_pruned_paths(b, eps, x0, n_steps, nb, n, k))
    if a["n_paths"] < 1:
        raise ValueError("eps must hold at least one baseline path")
    st = check_status(b.inp(status, "int32"), nb)
    girf = _out(b, out, (nb, c, n_steps, n))
    call(b, "dsge_girf_pruned_batched", **a, S_imp=impulses, s_batched=sb, c=c, status=st, girf_out=girf)
    return girf
