"""CPU: the front end of the stochastic simulation at an occasionally binding bound (``_frontend.constrained_simulate``) infers the
layouts of eps, c, bound and x0, refuses what is malformed or too large before anything is staged, and the library refuses the same
before any device is touched (this machine may have none)."""
import os
import re

import numpy as np
import pytest

from geconpy_amd import _lib, batched

NB, N, K, P = 2, 6, 3, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_OUTPUTS = ("duration", "iters", "path_status", "fail_step")


def _model(nb=NB, n=N, k=K):
    return np.zeros((nb, n, n)), np.zeros((nb, n, n)), np.zeros((nb, n, n)), np.zeros((nb, n, k))


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _NoCall())


class _Recorder:
    """Stands in for ``_lib.call``: keeps the named arguments of the one call."""

    def __call__(self, entry, *, host, stream=None, **named):
        self.entry, self.named = entry, named


@pytest.fixture
def recorded(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def test_layouts_and_output_shapes_are_inferred(recorded):
    call = batched.constrained_simulate_batched
    r = call(*_model(), np.zeros((4, 7, K)), np.ones(N), -0.5, 1, 9)  # eps, c and bound shared; the horizon beyond n_steps
    a = recorded.named
    assert recorded.entry == "dsge_constrained_simulate_batched"
    assert (a["eps_batched"], a["n_paths"], a["n_shock_steps"], a["n_steps"]) == (0, 4, 7, 7)
    assert (a["c_batched"], a["bound_batched"], a["shock"], a["horizon"], a["max_iter"], a["rank_tol"]) == (0, 0, 1, 9, 0, 0.0)
    assert (a["x0"], a["x0_batched"], a["x0_paths"], a["Z"], a["d"], a["p"]) == (None, 0, 0, None, None, 0)
    assert all(a[key] is None for key in ("obs_out", "gap_out", "shadow_out", "plan_out", "duration_out", "iters_out", "Mz_out",
                                          "path_status_out", "fail_step_out"))
    assert "w_out" not in a and "nu_out" not in a
    assert sorted(r) == ["status", "x"] and r["x"].shape == (NB, 4, 7, N) and r["status"].dtype == np.int32
    r = call(*_model(), np.zeros((NB, 4, 7, K)), np.ones((NB, N)), np.zeros(NB), 0, 5, n_steps=11, Z=np.eye(P, N), d=np.zeros((NB, P)),
             max_iter=9, rank_tol=1e-10, outputs=batched.F.OBC_SIM_OUTPUTS)
    a = recorded.named
    assert (a["eps_batched"], a["c_batched"], a["bound_batched"], a["n_steps"], a["max_iter"], a["rank_tol"]) == (1, 1, 1, 11, 9, 1e-10)
    assert (a["p"], a["z_batched"], a["d_batched"]) == (P, 0, 1)
    assert sorted(r) == sorted(batched.F.OBC_SIM_OUTPUTS + ("status",))
    assert batched.F.OBC_SIM_OUTPUTS == ("x", "observed", "gap", "shadow", "plan", "duration", "iters", "Mz", "path_status", "fail_step")
    assert r["x"].shape == (NB, 4, 11, N) and r["observed"].shape == (NB, 4, 11, P) and r["plan"].shape == (NB, 4, 11, 5)
    assert r["gap"].shape == r["shadow"].shape == r["duration"].shape == r["iters"].shape == (NB, 4, 11)
    assert r["Mz"].shape == (NB, 5, 5) and r["path_status"].shape == r["fail_step"].shape == (NB, 4)
    assert all(r[key].dtype == (np.int32 if key in INT_OUTPUTS else np.float64) for key in batched.F.OBC_SIM_OUTPUTS)
    call(*_model(), np.zeros((4, 7, K)), np.ones(N), np.array([0.25]), 0, 2, outputs="shadow")
    assert recorded.named["bound_batched"] == 0 and recorded.named["x_out"] is None and recorded.named["shadow_out"] is not None
    for x0, flags in ((np.zeros(N), (0, 0)), (np.zeros((4, N)), (0, 1)), (np.zeros((NB, 1, N)), (1, 0)), (np.zeros((NB, 4, N)), (1, 1))):
        call(*_model(), np.zeros((4, 7, K)), np.ones(N), 0.0, 0, 2, x0=x0)
        assert (recorded.named["x0_batched"], recorded.named["x0_paths"]) == flags, x0.shape


def test_every_refusal_comes_before_anything_is_staged(no_library):
    call = batched.constrained_simulate_batched
    eps, c = np.zeros((4, 7, K)), np.ones(N)
    with pytest.raises(ValueError, match="at most 64"):
        call(*_model(n=65), eps, np.ones(65), 0.0, 0, 2)
    with pytest.raises(ValueError, match="horizon = 0"):
        call(*_model(), eps, c, 0.0, 0, 0)
    with pytest.raises(ValueError, match="horizon = 65"):
        call(*_model(), eps, c, 0.0, 0, 65)
    with pytest.raises(ValueError, match="at least the 7 shock steps"):
        call(*_model(), eps, c, 0.0, 0, 2, n_steps=6)
    with pytest.raises(ValueError, match="shock = 3"):
        call(*_model(), eps, c, 0.0, K, 2)
    with pytest.raises(ValueError, match="shock = -1"):
        call(*_model(), eps, c, 0.0, -1, 2)
    with pytest.raises(ValueError, match="are needed"):
        call(*_model(), eps, None, 0.0, 0, 2)
    with pytest.raises(ValueError, match="are needed"):
        call(*_model(), eps, c, None, 0, 2)
    with pytest.raises(ValueError, match="c must be"):
        call(*_model(), eps, np.ones(N + 1), 0.0, 0, 2)
    with pytest.raises(ValueError, match="bound must be"):
        call(*_model(), eps, c, np.zeros(NB + 1), 0, 2)
    with pytest.raises(ValueError, match="outputs must name"):
        call(*_model(), eps, c, 0.0, 0, 2, outputs=())
    with pytest.raises(ValueError, match="outputs must name"):
        call(*_model(), eps, c, 0.0, 0, 2, outputs=("x", "w"))
    with pytest.raises(ValueError, match="outputs must name"):
        call(*_model(), eps, c, 0.0, 0, 2, outputs=("nu",))
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), np.zeros((4, 7, K + 1)), c, 0.0, 0, 2)
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), np.zeros((NB + 1, 4, 7, K)), c, 0.0, 0, 2)
    B, C, T, R = _model()
    with pytest.raises(ValueError, match="B and C must be"):
        call(B[:1], C, T, R, eps, c, 0.0, 0, 2)
    with pytest.raises(ValueError, match="x0 must be"):
        call(B, C, T, R, eps, c, 0.0, 0, 2, x0=np.zeros((3, N)))
    with pytest.raises(ValueError, match="need Z"):
        call(B, C, T, R, eps, c, 0.0, 0, 2, outputs=("observed",))
    with pytest.raises(ValueError, match="need Z"):
        call(B, C, T, R, eps, c, 0.0, 0, 2, d=np.zeros(P))
    with pytest.raises(ValueError, match="Z must be"):
        call(B, C, T, R, eps, c, 0.0, 0, 2, Z=np.eye(P, N + 1))
    with pytest.raises(ValueError, match="at most 16"):
        call(*_model(n=20), eps, np.ones(20), 0.0, 0, 2, Z=np.eye(17, 20))
    with pytest.raises(ValueError, match="status must be"):
        call(B, C, T, R, eps, c, 0.0, 0, 2, status=np.zeros(NB + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="an output buffer"):
        from geconpy_amd import _frontend as F

        F.constrained_simulate(F.HOST, "constrained_simulate_batched", B, C, T, R, eps, c, 0.0, 0, 2, n_steps=None, x0=None, Z=None,
                               d=None, status=None, rank_tol=0.0, max_iter=0, outputs=("plan",), out=dict(plan=np.empty((NB, 4, 7, 3))))


N_OUT = 10  # x, observed, gap, shadow, plan, duration, iters, Mz, path_status, fail_step


def _raw(B, C, T, R, *, n_steps=5, n_shock=5, n_paths=1, p=0, Z=None, eps="zeros", c="ones", bound="zero", shock=0, horizon=2,
         outs=(True,) + (False,) * (N_OUT - 1)):
    """The host twin called directly: the return code, with everything after the refusal never reached on a machine without a GPU."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nb, n, k = (NB, N, K) if R is None else R.shape
    eps = np.zeros((max(n_paths, 1), max(n_shock, 1), k)) if isinstance(eps, str) else eps
    c = np.ones(n) if isinstance(c, str) else c
    bound = np.zeros(1) if isinstance(bound, str) else bound
    size = nb * max(n_paths, 1) * max(n_steps, 1) * 64 + nb * 64 * 64
    bufs = [np.empty(size, dtype=np.int32 if i in (5, 6, 8, 9) else np.float64) if on else None for i, on in enumerate(outs)]
    return lib.dsge_constrained_simulate_batched_host(ptr(B), ptr(C), ptr(T), ptr(R), ptr(eps), 0, None, 0, 0, ptr(Z), 0, None, 0, ptr(c),
                                                      0, ptr(bound), 0, shock, horizon, 0, None, nb, n, k, p, n_paths, n_steps, n_shock,
                                                      0.0, *(ptr(b) for b in bufs))


def test_the_library_refuses_sizes_before_any_device():
    big, err = _lib.ERR_TOO_LARGE, lambda: _lib.load().dsge_last_error()  # noqa: E731
    assert _raw(*_model(n=65)) == big and b"DSGE_MAX_N" in err()
    assert _raw(*_model(n=20), p=17, Z=np.eye(17, 20)) == big and b"DSGE_MAX_P" in err()
    # no size the perfect-foresight entry accepts is refused: n = H = 64 with k = 32 and k = 64 go on to the device
    assert _raw(*_model(n=64, k=32), p=16, Z=np.eye(16, 64), n_steps=5, horizon=64) in (0, _lib.ERR_HIP)
    assert _raw(*_model(n=64, k=64), p=16, Z=np.eye(16, 64), n_steps=5, horizon=64) in (0, _lib.ERR_HIP)


def test_the_library_refuses_malformed_calls_before_any_device():
    bad, err = _lib.ERR_INVALID, lambda: _lib.load().dsge_last_error()  # noqa: E731
    B, C, T, R = _model()
    assert _raw(B, C, T, R, horizon=0) == bad and b"horizon" in err()
    assert _raw(B, C, T, R, horizon=65) == bad and b"horizon" in err()
    assert _raw(B, C, T, R, horizon=64, n_steps=5) in (0, _lib.ERR_HIP)  # the horizon bears no relation to n_steps
    assert _raw(B, C, T, R, n_steps=4, n_shock=5) == bad and b"n_shock_steps > n_steps" in err()
    assert _raw(B, C, T, R, n_steps=5, n_shock=5) in (0, _lib.ERR_HIP) and _raw(B, C, T, R, n_steps=6, n_shock=2) in (0, _lib.ERR_HIP)
    assert _raw(B, C, T, R, shock=K) == bad and b"shock" in err()
    assert _raw(B, C, T, R, shock=-1) == bad and _raw(B, C, T, R, shock=K - 1) in (0, _lib.ERR_HIP)
    assert _raw(B, C, T, R, c=None) == bad and b"null pointer" in err()
    assert _raw(B, C, T, R, bound=None) == bad and b"null pointer" in err()
    assert _raw(None, C, T, R) == bad and _raw(B, None, T, R) == bad and _raw(B, C, None, R) == bad and _raw(B, C, T, None) == bad
    assert _raw(B, C, T, R, eps=None) == bad and b"null pointer" in err()
    assert _raw(B, C, T, R, eps=None, n_shock=0) in (0, _lib.ERR_HIP)  # no shock at all needs no eps
    assert _raw(B, C, T, R, outs=(False,) * N_OUT) == bad and b"no output" in err()
    for i in range(2, N_OUT):  # every output besides x and observed alone is an output
        assert _raw(B, C, T, R, outs=tuple(j == i for j in range(N_OUT))) in (0, _lib.ERR_HIP)
    assert _raw(B, C, T, R, outs=(False, True) + (False,) * (N_OUT - 2)) == bad and b"p == 0" in err()  # observed without Z
    assert _raw(B, C, T, R, p=2) == bad and b"without Z" in err()
    assert _raw(*_model(n=3, k=4)) == bad
    assert _raw(B, C, T, R, n_steps=-1) == bad and _raw(B, C, T, R, n_paths=-1) == bad
    # the empty call: success, nothing touched
    assert _raw(B, C, T, R, n_paths=0) in (0, _lib.ERR_HIP) and _raw(B, C, T, R, n_steps=0, n_shock=0) in (0, _lib.ERR_HIP)


def test_abi_version_and_constants_match_the_header():
    assert _lib.ABI_VERSION == 19
    text = open(os.path.join(ROOT, "include", "dsge_hip.h")).read()
    consts = dict(re.findall(r"#define\s+(DSGE_[A-Z_0-9]+)\s+(-?\d+)", text))
    assert int(consts["DSGE_ABI_VERSION"]) == _lib.ABI_VERSION
    assert int(consts["DSGE_OBC_HORIZON_SHORT"]) == _lib.OBC_HORIZON_SHORT == 16
    assert int(consts["DSGE_OBC_NO_REGIME"]) == _lib.OBC_NO_REGIME and int(consts["DSGE_OBC_SINGULAR"]) == _lib.OBC_SINGULAR
    assert int(consts["DSGE_OBC_SKIPPED"]) == _lib.OBC_SKIPPED and int(consts["DSGE_OBC_MAX_HORIZON"]) == _lib.OBC_MAX_HORIZON
    assert int(consts["DSGE_ST_CONSTRAINT_UNRESOLVED"]) == _lib.ST_CONSTRAINT_UNRESOLVED
    assert re.search(r"/\* ABI 19: dsge_constrained_simulate_batched .* new; nothing else changed\. \*/", text)
    sig = [name for name, _ in _lib.SIGNATURES["dsge_constrained_simulate_batched"]]
    assert sig[-1] == "stream" and [name for name, _ in _lib.SIGNATURES["dsge_constrained_simulate_batched_host"]] == sig[:-1]
    # the arguments of the perfect-foresight entry first, in its order, without w_out and nu_out
    pf = [name for name, _ in _lib.SIGNATURES["dsge_constrained_paths_batched"]]
    head = pf[:pf.index("x_out")]
    assert sig[:len(head)] == head
    assert sig[len(head):-1] == ["x_out", "obs_out", "gap_out", "shadow_out", "plan_out", "duration_out", "iters_out", "Mz_out",
                                 "path_status_out", "fail_step_out"]


def test_no_kernel_of_the_entry_spills_to_scratch_memory(tmp_path):
    """The simulation kernel keeps the regime iteration's row of up to 64 entries of K per lane in registers next to its own state of
    the time loop; a compiler that starts to spill either must not go unnoticed."""
    import subprocess

    from geconpy_amd import build

    out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "a.o"),
                          os.path.join(build.CSRC, "launch_obc_sim.hip")], cwd=build.CSRC, capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S*obc_sim\S*kernel\S*)", out.stderr)
    sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len({n for n in names if "obc_sim_kernel" in n}) == 2 and len({n for n in names if "obc_sim_setup_kernel" in n}) == 1
    assert len(sizes) >= 3 and set(sizes) == {"0"}
