"""CPU: the Python front-end above the C ABI -- the named caller of ``_lib``, the shape / layout description both backends share
(``_frontend``), and the arguments the numpy front-end hands to the library, pinned by tests/golden/call_args.json."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest

from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_call_args_golden", os.path.join(GOLDEN, "make_call_args_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(recorder.FIXTURE) as _f:
    PINNED = json.load(_f)  # written from the commit before the front-end was rewritten; never by the code under test


def test_the_fixture_covers_every_paired_entry():
    entries = {call[0] for calls in PINNED.values() for call in calls}
    assert entries >= {"dsge_solve_kalman_logp_batched_host_opt", "dsge_solve_kalman_logp_grad_batched_host_opt",
                       "dsge_solve_kalman_logp_grad_dense_z_batched_host", "dsge_kalman_smoother_batched_host",
                       "dsge_simulate_batched_host", "dsge_irf_batched_host", "dsge_forecast_batched_host",
                       "dsge_second_order_logp_batched_host"}
    assert [label for label, _ in recorder.cases()] == list(PINNED)


@pytest.mark.parametrize("label", list(PINNED))
def test_host_calls_are_the_pinned_ones(label):
    """Entry, every scalar and the null-ness of every pointer of each library call the public ``batched`` function makes."""
    assert recorder.record(dict(recorder.cases())[label]) == PINNED[label]


def test_device_calls_are_the_host_calls_plus_the_stream(monkeypatch):
    """The same front-end with ``host = False`` (the one switch a backend flips) reaches the device entry with the same arguments
    and a trailing stream -- second order also takes ``stage_ms`` there."""
    monkeypatch.setattr(F.HostBackend, "host", False)
    for label, fn in recorder.cases():
        want = []
        for entry, *args in PINNED[label]:
            if "_host" in entry:
                entry = entry.replace("_host", "")
                args = args + ["null"] * (2 if entry == "dsge_second_order_logp_batched" else 1)
            want.append([entry, *args])
        assert recorder.record(fn) == want, label


def test_named_caller():
    rec = recorder.Recorder()
    saved, _lib._lib = _lib._lib, rec
    try:
        args = dict(T=1, R=2, Q=3, q_mode=np.int64(1), batch=3, m=5, k=2, P0_out=4, RQR_out=5, status=6)
        _lib.call("dsge_lyapunov_batched", host=True, **args)
        _lib.call("dsge_lyapunov_batched", host=False, stream=7, **dict(reversed(args.items())))
        assert rec.calls == [["dsge_lyapunov_batched_host", "ptr", "ptr", "ptr", 1, 3, 5, 2, "ptr", "ptr", "ptr"],
                             ["dsge_lyapunov_batched", "ptr", "ptr", "ptr", 1, 3, 5, 2, "ptr", "ptr", "ptr", "ptr"]]
        assert type(rec.calls[0][4]) is int
        with pytest.raises(TypeError, match="missing .'status'., unknown .'stat'."):
            _lib.call("dsge_lyapunov_batched", host=True, **{**{k: v for k, v in args.items() if k != "status"}, "stat": 6})
        with pytest.raises(TypeError, match="missing .'m'."):
            _lib.call("dsge_lyapunov_batched", host=False, **{k: v for k, v in args.items() if k != "m"})
        with pytest.raises(TypeError, match="takes no stream"):  # a host twin has none: only None passes
            _lib.call("dsge_lyapunov_batched", host=True, stream=7, **args)
        assert len(rec.calls) == 2
    finally:
        _lib._lib = saved


def test_scalars_may_be_numpy_scalars():
    """A scalar argument is a scalar by the table, whatever the value looks like: numpy scalars and 0-d arrays (values read out of
    arrays or configs) reach the library as the plain Python numbers do, through every paired public function."""
    nb, n, k, p, T_len = recorder.NB, recorder.N, recorder.K, recorder.P, recorder.T_LEN
    M, D, y, Z, q = np.zeros((nb, n, n)), np.zeros((nb, n, k)), np.zeros((T_len, p)), np.eye(p, n), np.ones(k)
    a0, eps, idx, val = np.zeros((nb, n)), np.zeros((2, 3, k)), np.zeros((4, 3), dtype=np.int32), np.zeros((nb, 4))
    solve = dict(tol=1e-7, max_iter=9, jitter=1e-9, missing_fill_value=-99.0)
    calls = {
        "logp": (lambda **kw: batched.solve_kalman_logp_batched(M, M, M, D, q, Z, y, **kw),
                 dict(solve, n_state_hint=4, z_selector_hint=1, n_lead_hint=2)),
        "grad": (lambda **kw: batched.solve_kalman_logp_grad_batched(M, M, M, D, q, Z, y, **kw),
                 dict(solve, n_filter_hint=4, n_lead_hint=2)),
        "dense grad": (lambda **kw: batched.solve_kalman_logp_grad_batched(M, M, M, D, q, Z, y, dense_z=True, **kw),
                       dict(solve, n_filter_hint=3, n_lead_hint=2)),
        "second order": (lambda **kw: batched.second_order_logp_batched(M, M, M, D, idx, val, q, Z, y, **kw), solve),
        "smoother": (lambda **kw: batched.kalman_smoother_batched(M, D, q, Z, y, **kw),
                     dict(jitter=1e-9, missing_fill_value=-99.0, rank_tol=1e-9, scratch_limit_bytes=1 << 20)),
        "simulate": (lambda **kw: batched.simulate_batched(M, D, eps, **kw), dict(n_steps=5)),
        "irf": (lambda **kw: batched.impulse_response_batched(M, D, **kw), dict(n_steps=5)),
        "forecast": (lambda **kw: batched.forecast_batched(M, D, q, a0, **kw), dict(n_steps=5)),
    }
    for name, (fn, scalars) in calls.items():
        plain = recorder.record(lambda: fn(**scalars))
        assert len(plain) == 1 and all(type(v) in (int, float, str) for v in plain[0]), name
        for wrap in (lambda v: np.array(v)[()], np.array):  # a numpy scalar; a 0-d array
            assert recorder.record(lambda: fn(**{key: wrap(v) for key, v in scalars.items()})) == plain, name


def test_layouts_from_shapes_alone():
    class Shape:  # anything with .shape will do: numpy array or torch tensor
        def __init__(self, *shape):
            self.shape = shape

    nb, k, p, m = 3, 2, 2, 5
    for name, shape in (("diag", (k,)), ("diag_batched", (nb, k)), ("full", (k, k)), ("full_batched", (nb, k, k))):
        for q_mode in (None, name, F.Q_MODES[name]):
            assert F.q_layout(shape, q_mode, nb, k) == F.Q_MODES[name]
        for other in F.Q_MODES:
            if other != name:
                with pytest.raises(ValueError, match="q_mode needs"):
                    F.q_layout(shape, other, nb, k)
    assert F.q_layout((k, k), "diag_batched", k, k) == _lib.Q_DIAG_BATCHED and F.q_layout((k, k), "full", k, k) == _lib.Q_FULL_SHARED
    for shape in ((k + 1,), (nb, k + 1), (nb + 1, k), (k, k, k), ()):
        with pytest.raises(ValueError, match="cannot infer the layout of Q"):
            F.q_layout(shape, None, nb, k)
    assert [F.grad_q_layout(s, f, nb, k) for s, f in (((k,), False), ((nb, k), False), ((k, k), True), ((nb, k, k), True))] == [0, 1, 2, 3]
    for shape, full in (((k, k), False), ((nb, k, k), False), ((k,), True), ((nb, k), True), ((k + 1,), False)):
        with pytest.raises(ValueError, match="must be"):
            F.grad_q_layout(shape, full, nb, k)
    assert F.obs_flags(Shape(p, m), None, None, nb, p, m) == (0, 0, 0)
    assert F.obs_flags(Shape(nb, p, m), Shape(p), Shape(nb, p), nb, p, m) == (1, 0, 1)
    assert F.obs_flags(Shape(p, m), Shape(nb, p), Shape(p), nb, p, m) == (0, 1, 0)
    for Z, d, H, what in ((Shape(p, m - 1), None, None, "Z"), (Shape(nb + 1, p, m), None, None, "Z"),
                          (Shape(p, m), Shape(p + 1), None, "d"),
                          (Shape(p, m), None, Shape(nb + 1, p), "Hdiag"), (Shape(p, m), Shape(nb, p, 1), None, "d")):
        with pytest.raises(ValueError, match=f"{what} must be"):
            F.obs_flags(Z, d, H, nb, p, m)
    assert F.shared_or_batched(Shape(4, k), nb, (4, k), "S") == 0 and F.shared_or_batched(Shape(nb, 4, k), nb, (4, k), "S") == 1
    with pytest.raises(ValueError, match=r"S must be \(4, 2\) or \(3, 4, 2\); got \(2, 4\)"):
        F.shared_or_batched(Shape(k, 4), nb, (4, k), "S")
    assert F.check_status(None, nb) is None
    with pytest.raises(ValueError, match="status must be"):
        F.check_status(Shape(nb + 1), nb)
    assert [F.cov_flags(c) for c in ("diag", "full", None)] == [(True, False), (True, True), (False, False)]
    with pytest.raises(ValueError):
        F.cov_flags("both")


class CheckOnly(F.HostBackend):
    """What the device backend is to the shared front-end: inputs are checked, never coerced, and the device entry is called."""

    host = False

    @staticmethod
    def inp(x, dtype="float64"):
        assert x is None or x.dtype == np.dtype(dtype)
        return x


NB, N, K, P, T_LEN = recorder.NB, recorder.N, recorder.K, recorder.P, recorder.T_LEN


def _front_end(b):
    """name -> f(**overrides): the shared front-end of backend ``b`` on one small well-formed problem, changed in ``overrides``."""
    M, D = np.zeros((NB, N, N)), np.zeros((NB, N, K))
    base = dict(T=M, R=D, Q=np.ones(K), full=False, Z=np.eye(P, N), y=np.zeros((T_LEN, P)), d=None, Hdiag=None, q_mode=None, status=None,
                out=None, limit=None, eps=np.zeros((2, 3, K)), x0=None, n_steps=3, S=None, weights=None, fevd=False, irf=True,
                a0=np.zeros((NB, N)), P0=None, covariances="diag", idx=np.zeros((4, 3), dtype=np.int32), val=np.zeros((NB, 4)))
    solve = dict(solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=1e-8, missing_fill=-9999.0, options=None)
    hints = lambda a: dict(n_state_hint=0, z_selector_hint=0, n_lead_hint=0)  # noqa: E731
    route = lambda a: dict(dense_z=False, Z_bar=False, n_hint=0, n_lead_hint=0)  # noqa: E731
    entries = {
        "logp": lambda v: F.solve_kalman_logp(b, M, M, M, D, v.Q, v.Z, v.y, d=v.d, Hdiag=v.Hdiag, q_mode=v.q_mode, hints=hints, out=v.out,
                                              **solve),
        "grad": lambda v: F.solve_kalman_logp_grad(b, M, M, M, D, v.Q, v.Z, v.y, full=v.full, d=v.d, Hdiag=v.Hdiag, route=route, out=v.out,
                                                   **solve),
        "second order": lambda v: F.second_order_logp(b, M, M, M, D, v.idx, v.val, v.Q, v.Z, v.y, d=v.d, Hdiag=v.Hdiag,
                                                      structure=([0], [1], [0]), **solve),
        "smoother": lambda v: F.kalman_smoother(b, "smoother", v.T, v.R, v.Q, v.Z, v.y, d=v.d, Hdiag=v.Hdiag, q_mode=v.q_mode,
                                                status=v.status, jitter=1e-8, missing_fill=-9999.0, cov=True, full=False, rank_tol=None,
                                                scratch_limit_bytes=v.limit, options=None),
        "simulate": lambda v: F.simulate(b, "simulate", v.T, v.R, v.eps, n_steps=v.n_steps, x0=v.x0, status=v.status),
        "irf": lambda v: F.impulse_response(b, "irf", v.T, v.R, n_steps=v.n_steps, S=v.S, weights=v.weights, fevd=v.fevd, irf=v.irf,
                                            status=v.status),
        "forecast": lambda v: F.forecast(b, "forecast", v.T, v.R, v.Q, v.a0, P0=v.P0, n_steps=v.n_steps, Z=v.Z, d=v.d, Hdiag=v.Hdiag,
                                         q_mode=v.q_mode, covariances=v.covariances, status=v.status),
    }
    return {name: (lambda fn=fn, **kw: fn(types.SimpleNamespace(**{**base, **kw}))) for name, fn in entries.items()}


_OBSERVATION = [("d of (p + 1,)", dict(d=np.zeros(P + 1))), ("Z of (p, m - 1)", dict(Z=np.eye(P, N - 1))),
                ("Hdiag of (batch + 1, p)", dict(Hdiag=np.ones((NB + 1, P)))), ("Z of (batch + 1, p, m)", dict(Z=np.zeros((NB + 1, P, N))))]
_STATUS = [("status of the wrong length", dict(status=np.zeros(NB + 1, dtype=np.int32)))]
_MALFORMED = {  # entry -> (what is wrong, the arguments that make it so)
    "logp": _OBSERVATION + [("Q of (k + 1,)", dict(Q=np.ones(K + 1))), ("q_mode against the shape", dict(q_mode="full")),
                            ("y 1-d", dict(y=np.zeros(P))), ("an output buffer too short", dict(out=dict(logp=np.zeros(NB - 1))))],
    "grad": _OBSERVATION + [("q full but not told so", dict(Q=np.eye(K))), ("Q diagonal but told full", dict(full=True)),
                            ("a reused buffer of another layout", dict(out=dict(q_bar=np.zeros((NB, K, K)))))],
    "second order": [("hess_val", dict(val=np.zeros((NB, 5)))), ("hess_idx", dict(idx=np.zeros((4, 2), dtype=np.int32))),
                     ("q full", dict(Q=np.eye(K))), ("Z batched", dict(Z=np.zeros((NB, P, N)))), ("d of (p + 1,)", dict(d=np.zeros(P + 1))),
                     ("Hdiag batched", dict(Hdiag=np.ones((NB, P))))],
    "smoother": _OBSERVATION + _STATUS + [("T not square", dict(T=np.zeros((NB, N, N + 1)))),
                                          ("R of another batch", dict(R=np.zeros((NB + 1, N, K)))),
                                          ("m = 65", dict(T=np.zeros((1, 65, 65)), R=np.zeros((1, 65, K)))),
                                          ("negative scratch limit", dict(limit=-1))],
    "simulate": _STATUS + [("eps of another k", dict(eps=np.zeros((2, 3, K + 1)))),
                           ("eps of another batch", dict(eps=np.zeros((NB + 1, 2, 3, K)))),
                           ("fewer steps than shocks", dict(n_steps=2)), ("x0", dict(x0=np.zeros((3, N)))),
                           ("m = 97", dict(T=np.zeros((1, 97, 97)), R=np.zeros((1, 97, K)))),
                           ("k = 0", dict(R=np.zeros((NB, N, 0)), eps=np.zeros((2, 3, 0))))],
    "irf": _STATUS + [("S of another k", dict(S=np.zeros((K + 1, 3)))), ("weights", dict(S=np.zeros((K, 3)), weights=np.ones(K))),
                      ("nothing requested", dict(irf=False)), ("negative steps", dict(n_steps=-1))],
    "forecast": _OBSERVATION + _STATUS + [("a0", dict(a0=np.zeros((NB, N + 1)))), ("P0", dict(P0=np.zeros((NB, N, N + 1)))),
                                          ("covariances", dict(covariances="both")), ("d without Z", dict(Z=None, d=np.zeros(P))),
                                          ("negative steps", dict(n_steps=-1))],
}


@pytest.mark.parametrize("backend", ["host", "device"])
def test_malformed_calls_are_value_errors_for_both_backends(backend):
    """Every malformed case is refused before the library is reached -- by the numpy backend and by one that, like the device
    backend, only checks its inputs (a wrong shape there used to be an out-of-bounds read on the device)."""
    entries = _front_end(F.HOST if backend == "host" else CheckOnly())
    rec = recorder.Recorder()
    saved, _lib._lib = _lib._lib, rec
    try:
        for fn in entries.values():
            fn()
        assert [c[0] for c in rec.calls if "options" not in c[0]] == [
            e if backend == "device" else _lib.host_twin(e) for e in (
                "dsge_solve_kalman_logp_batched_opt", "dsge_solve_kalman_logp_grad_batched_opt", "dsge_second_order_logp_batched",
                "dsge_kalman_smoother_batched", "dsge_simulate_batched", "dsge_irf_batched", "dsge_forecast_batched")]
        n_calls = len(rec.calls)
        for name, cases in _MALFORMED.items():
            for what, change in cases:
                with pytest.raises(ValueError):
                    entries[name](**change)
                    pytest.fail(f"{name}: {what}: accepted")
        assert len(rec.calls) == n_calls
    finally:
        _lib._lib = saved


def test_malformed_calls_through_the_public_numpy_functions():
    """The cases ``batched`` rejected before the front-end was shared are still ValueErrors, with their messages."""
    nb, n, k, p, T_len = 3, 5, 2, 2, 4
    M, D, y, Z, q = np.zeros((nb, n, n)), np.zeros((nb, n, k)), np.zeros((T_len, p)), np.eye(p, n), np.ones(k)
    a0, eps = np.zeros((nb, n)), np.zeros((2, 3, k))
    cases = [
        (r"A, B, C must be \(batch, n, n\)", lambda: batched.solve_kalman_logp_batched(M, M[:, :4], M, D, q, Z, y)),
        ("expected a 3-d array", lambda: batched.solve_kalman_logp_batched(M, M, M, D[0], q, Z, y)),
        ("expected a 2-d array", lambda: batched.solve_kalman_logp_grad_batched(M, M, M, D, q, Z, y[0])),
        ("cannot infer the layout of Q", lambda: batched.solve_kalman_logp_batched(M, M, M, D, np.ones(k + 1), Z, y)),
        (r"Q has shape \(2,\), q_mode needs \(2, 2\)", lambda: batched.kalman_smoother_batched(M, D, q, Z, y, q_mode="full")),
        (r"Z must be \(p, m\) or \(batch, p, m\); got \(2, 4\)", lambda: batched.solve_kalman_logp_batched(M, M, M, D, q, Z[:, :4], y)),
        (r"d must be \(p,\) or \(batch, p\); got \(3,\)", lambda: batched.kalman_smoother_batched(M, D, q, Z, y, d=np.zeros(p + 1))),
        (r"Hdiag must be \(p,\) or \(batch, p\); got \(4, 2\)",
         lambda: batched.forecast_batched(M, D, q, a0, Z=Z, Hdiag=np.ones((nb + 1, p)))),
        ("pass either q", lambda: batched.solve_kalman_logp_grad_batched(M, M, M, D, q, Z, y, Q=np.eye(k))),
        (r"Q must be \(k, k\) or \(batch, k, k\)", lambda: batched.solve_kalman_logp_grad_batched(M, M, M, D, None, Z, y, Q=q)),
        (r"q must be \(k,\) or \(batch, k\) \(diagonal shock covariance\)",
         lambda: batched.solve_kalman_logp_grad_batched(M, M, M, D, np.eye(k), Z, y)),
        (r"hess_val must be \(batch, nnz\)",
         lambda: batched.second_order_logp_batched(M, M, M, D, np.zeros((4, 3)), np.zeros((nb, 5)), q, Z, y)),
        (r"Z must be \(p, n\)", lambda: batched.second_order_logp_batched(M, M, M, D, np.zeros((4, 3)), np.zeros((nb, 4)), q, Z[:, :4], y)),
        ("expected a 1-d array",
         lambda: batched.second_order_logp_batched(M, M, M, D, np.zeros((4, 3)), np.zeros((nb, 4)), q, Z, y, d=np.zeros((nb, p)))),
        (r"T must be \(batch, m, m\) and R \(batch, m, k\)", lambda: batched.kalman_smoother_batched(M, D[:2], q, Z, y)),
        ("kalman_smoother_batched: m = 65, the smoother takes at most 64 variables",
         lambda: batched.kalman_smoother_batched(np.zeros((1, 65, 65)), np.zeros((1, 65, k)), q, np.eye(p, 65), y)),
        ("scratch_limit_bytes must be >= 0", lambda: batched.kalman_smoother_batched(M, D, q, Z, y, scratch_limit_bytes=-1)),
        (r"status must be \(batch,\); got \(4,\)", lambda: batched.kalman_smoother_batched(M, D, q, Z, y, status=np.zeros(nb + 1))),
        (r"status must be \(batch,\); got \(2,\)", lambda: batched.simulate_batched(M, D, eps, status=np.zeros(nb - 1))),
        ("simulate_batched: m = 97, at most 96 variables",
         lambda: batched.simulate_batched(np.zeros((1, 97, 97)), np.zeros((1, 97, k)), eps)),
        (r"eps must be \(n_paths, n_shock_steps, 2\) or \(batch, n_paths, n_shock_steps, 2\); got \(2, 3, 3\)",
         lambda: batched.simulate_batched(M, D, np.zeros((2, 3, k + 1)))),
        (r"eps must be \(2, 3, 2\) or \(3, 2, 3, 2\); got \(4, 2, 3, 2\)",
         lambda: batched.simulate_batched(M, D, np.zeros((nb + 1, 2, 3, k)))),
        ("n_steps = 2 is less than the 3 shock steps of eps", lambda: batched.simulate_batched(M, D, eps, n_steps=2)),
        (r"x0 must be \(2, 5\) or \(3, 2, 5\); got \(3, 5\)", lambda: batched.simulate_batched(M, D, eps, x0=np.zeros((3, n)))),
        (r"S must be \(2, c\) or \(batch, 2, c\); got \(3, 3\)", lambda: batched.impulse_response_batched(M, D, S=np.zeros((k + 1, 3)))),
        (r"weights must be \(3,\) or \(3, 3\); got \(2,\)",
         lambda: batched.impulse_response_batched(M, D, S=np.zeros((k, 3)), weights=np.ones(k))),
        ("nothing requested", lambda: batched.impulse_response_batched(M, D, irf=False)),
        ("n_steps must be >= 0", lambda: batched.impulse_response_batched(M, D, n_steps=-1)),
        (r"a0 must be \(3, 5\); got \(3, 6\)", lambda: batched.forecast_batched(M, D, q, np.zeros((nb, n + 1)))),
        (r"P0 must be \(3, 5, 5\); got \(3, 5, 6\)", lambda: batched.forecast_batched(M, D, q, a0, P0=np.zeros((nb, n, n + 1)))),
        ('covariances must be "diag", "full" or None', lambda: batched.forecast_batched(M, D, q, a0, covariances="both")),
        ("d and Hdiag need Z", lambda: batched.forecast_batched(M, D, q, a0, d=np.zeros(p))),
        ("n_steps must be >= 0", lambda: batched.forecast_batched(M, D, q, a0, n_steps=-1)),
    ]
    for match, fn in cases:
        with pytest.raises(ValueError, match=match):
            recorder.record(fn)
