"""The arguments the numpy front-end hands to the C ABI, recorded without a GPU: call_args.json.

A recorder stands in for the loaded library (``_lib._lib``; every entry returns 0) while the public ``batched`` functions of the
seven entry points that also have a device front-end are driven over the shock-covariance layouts, the observation-model
variants, ``status`` given or not, the covariance settings, the gradient's ``q`` / ``Q=`` / dense-Z routes and second order with
and without the solution.  Per call it keeps the entry name, every scalar argument and whether each pointer argument is null.

The fixture pins the front-end's behaviour across refactors, so it is written from the commit BEFORE a change to the front-end
(``python tests/golden/make_call_args_golden.py``) and only replayed afterwards (tests/test_frontend.py).
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from geconpy_amd import _lib, batched  # noqa: E402

FIXTURE = os.path.join(HERE, "call_args.json")
NB, N, K, P, T_LEN = 3, 5, 2, 2, 4  # batch != k: the layout of Q is inferred without ambiguity


class Recorder:
    """Stands in for the ctypes handle: ``recorder.dsge_x(*args)`` notes the call and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, entry):
        argtypes = _lib.PROTOTYPES[entry]

        def fn(*args):
            assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
            self.calls.append([entry] + [("null" if a in (None, 0) else "ptr") if t is ctypes.c_void_p else a
                                         for a, t in zip(args, argtypes)])
            return 0

        return fn


def record(fn):
    """The library calls ``fn()`` makes, as JSON-ready lists ``[entry, arg, ...]``."""
    saved, rec = _lib._lib, Recorder()
    _lib._lib = rec
    try:
        fn()
    finally:
        _lib._lib = saved
    return json.loads(json.dumps(rec.calls))


def cases():
    """(label, thunk) for every pinned call."""
    rng = np.random.default_rng(0)
    A, B, C = (rng.standard_normal((NB, N, N)) for _ in range(3))
    A[:, :, 3:] = 0.0  # three state variables
    C[:, :, :2] = 0.0
    D = rng.standard_normal((NB, N, K))
    T, R = 0.1 * rng.standard_normal((NB, N, N)), D
    y = rng.standard_normal((T_LEN, P))
    Zs = np.eye(P, N)  # a selector
    Zd = Zs + 0.5 * np.eye(P, N, 1)  # not a selector
    tile = lambda x: np.broadcast_to(x, (NB, *x.shape)).copy()  # noqa: E731
    dv, hv = np.full(P, 0.1), np.full(P, 0.01)
    st = np.zeros(NB, dtype=np.int32)
    Qs = {"diag": np.ones(K), "diag_batched": np.ones((NB, K)), "full": np.eye(K), "full_batched": tile(np.eye(K))}
    obs = dict(absent={}, shared=dict(d=dv, Hdiag=hv), batched=dict(d=tile(dv), Hdiag=tile(hv)))
    a0 = rng.standard_normal((NB, N))
    P0 = tile(np.eye(N))
    out = []
    add = lambda label, fn, *a, **kw: out.append((label, lambda: fn(*a, **kw)))  # noqa: E731

    for name, Q in Qs.items():
        for qm in (None, name):
            tag = f"Q={name},q_mode={qm}"
            add(f"logp {tag}", batched.solve_kalman_logp_batched, A, B, C, D, Q, Zs, y, q_mode=qm)
            add(f"smoother {tag}", batched.kalman_smoother_batched, T, R, Q, Zs, y, q_mode=qm)
            add(f"forecast {tag}", batched.forecast_batched, T, R, Q, a0, q_mode=qm)
    for zname, Z in (("Z shared", Zs), ("Z batched", tile(Zs)), ("Z dense", Zd)):
        for oname, o in obs.items():
            tag = f"{zname}, d/Hdiag {oname}"
            add(f"logp {tag}", batched.solve_kalman_logp_batched, A, B, C, D, Qs["diag"], Z, y, **o)
            add(f"smoother {tag}", batched.kalman_smoother_batched, T, R, Qs["diag"], Z, y, **o)
            add(f"forecast {tag}", batched.forecast_batched, T, R, Qs["diag"], a0, Z=Z, **o)
            add(f"grad {tag}", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs["diag"], Z, y, **o)
    add("logp policy gensys", batched.solve_kalman_logp_batched, A, B, C, D, Qs["diag"], Zs, y, return_policy=True, solver="gensys",
        add_solver_success_check=False, options={"kalman_order": 2})
    add("logp hints given", batched.solve_kalman_logp_batched, A, B, C, D, Qs["diag"], Zs, y, n_state_hint=4, z_selector_hint=0,
        n_lead_hint=2, tol=1e-9, max_iter=7, jitter=0.0, missing_fill_value=-1.0)
    for full in (False, True):
        for status in (None, st):
            add(f"smoother full={full} status={status is not None}", batched.kalman_smoother_batched, T, R, Qs["full"], Zs, y,
                full_covariances=full, status=status, rank_tol=1e-9, scratch_limit_bytes=1 << 20)
    for cov in ("diag", "full", None):
        for status in (None, st):
            add(f"forecast cov={cov} status={status is not None}", batched.forecast_batched, T, R, Qs["diag_batched"], a0, P0=P0,
                n_steps=3, Z=Zs, Hdiag=hv, covariances=cov, status=status)
            add(f"forecast states only cov={cov} status={status is not None}", batched.forecast_batched, T, R, Qs["full"], a0,
                covariances=cov, status=status)
    eps = rng.standard_normal((2, 3, K))
    x0 = rng.standard_normal((2, N))
    for ename, e in (("shared", eps), ("batched", tile(eps))):
        for xname, x in (("none", None), ("shared", x0), ("batched", tile(x0))):
            for status in (None, st):
                add(f"simulate eps {ename} x0 {xname} status={status is not None}", batched.simulate_batched, T, R, e, x0=x,
                    status=status)
    add("simulate n_steps", batched.simulate_batched, T, R, eps, n_steps=6)
    S = rng.standard_normal((K, 3))
    for sname, s in (("none", None), ("shared", S), ("batched", tile(S))):
        c = K if s is None else 3
        for wname, w in (("none", None), ("shared", np.ones(c)), ("batched", np.ones((NB, c)))):
            for status in (None, st):
                add(f"irf S {sname} weights {wname} status={status is not None}", batched.impulse_response_batched, T, R, 5, S=s,
                    weights=w, fevd=True, status=status)
    add("irf only", batched.impulse_response_batched, T, R)
    add("fevd only", batched.impulse_response_batched, T, R, 4, fevd=True, irf=False)
    for qname in ("diag", "diag_batched"):
        add(f"grad q {qname}", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs[qname], Zs, y, d=dv, Hdiag=hv)
        add(f"grad q {qname} dense", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs[qname], Zd, y, d=dv)
    for qname in ("full", "full_batched"):
        add(f"grad Q= {qname}", batched.solve_kalman_logp_grad_batched, A, B, C, D, None, Zs, y, Q=Qs[qname], Hdiag=hv)
        add(f"grad Q= {qname} dense", batched.solve_kalman_logp_grad_batched, A, B, C, D, None, Zd, y, Q=Qs[qname])
    add("grad dense forced", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs["diag"], Zs, y, dense_z=True)
    add("grad Z_bar", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs["diag"], Zs, y, return_Z_bar=True,
        options={"kalman_grad_split": 1})
    add("grad hints given", batched.solve_kalman_logp_grad_batched, A, B, C, D, Qs["diag"], Zs, y, n_filter_hint=4, n_lead_hint=1,
        solver="gensys", options={"kalman_grad_split": 1})
    idx = np.array([[0, 0, 1], [1, 2, 2], [3, 0, 4]], dtype=np.int32)
    val = rng.standard_normal((NB, len(idx)))
    for sol in (False, True):
        for qname in ("diag", "diag_batched"):
            add(f"second order solution={sol} q {qname}", batched.second_order_logp_batched, A, B, C, D, idx, val, Qs[qname], Zs, y,
                return_solution=sol)
    add("second order d Hdiag", batched.second_order_logp_batched, A, B, C, D, idx, val, Qs["diag"], Zs, y, d=dv, Hdiag=hv,
        options={"kalman_order": 2})
    add("second order structure", batched.second_order_logp_batched, A, B, C, D, idx, val, Qs["diag"], Zs, y,
        structure=([0, 1], [2, 3, 4], [0, 1, 2]), solver="gensys")
    return out


def record_all():
    return {label: record(fn) for label, fn in cases()}


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        rows = [f"{json.dumps(label)}: {json.dumps(calls, separators=(',', ':'))}" for label, calls in record_all().items()]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print("wrote", FIXTURE)
