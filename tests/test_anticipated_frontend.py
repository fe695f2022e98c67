"""CPU: the front end of the anticipated-shock paths (``_frontend.anticipated_paths``) infers the layouts of eps and x0, refuses
what is malformed or too large before anything is staged, and the library refuses the same before any device is touched (this
machine may have none)."""
import os
import re

import numpy as np
import pytest

from geconpy_amd import _lib, batched

NB, N, K, P = 2, 6, 3, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_layouts_of_eps_and_x0_are_inferred(recorded):
    call = batched.anticipated_paths_batched
    r = call(*_model(), np.zeros((4, 7, K)), n_steps=5)  # perfect foresight, eps shared by the draws, beyond the horizon
    a = recorded.named
    assert recorded.entry == "dsge_anticipated_paths_batched"
    assert (a["mode"], a["n_lead"], a["eps_batched"], a["n_paths"], a["n_shock_steps"], a["n_steps"]) == (0, 0, 0, 4, 7, 5)
    assert (a["x0"], a["x0_batched"], a["x0_paths"], a["Z"], a["d"], a["p"]) == (None, 0, 0, None, None, 0)
    assert (a["batch"], a["n"], a["k"]) == (NB, N, K) and a["w_out"] is None and a["obs_out"] is None and a["G_out"] is None
    assert sorted(r) == ["status", "x"] and r["x"].shape == (NB, 4, 5, N) and r["status"].dtype == np.int32
    call(*_model(), np.zeros((NB, 4, 7, K)))  # per draw; n_steps defaults to the shock steps
    assert (recorded.named["eps_batched"], recorded.named["n_steps"]) == (1, 7)
    r = call(*_model(), np.zeros((4, 5, 3, K)), mode="news", n_steps=6, Z=np.eye(P, N), d=np.zeros((NB, P)),
             outputs=("w", "observed", "G"))
    a = recorded.named
    assert (a["mode"], a["n_lead"], a["eps_batched"], a["n_paths"], a["n_shock_steps"], a["n_steps"]) == (1, 2, 0, 4, 5, 6)
    assert (a["p"], a["z_batched"], a["d_batched"]) == (P, 0, 1) and a["x_out"] is None
    assert sorted(r) == ["G", "observed", "status", "w"]
    assert r["w"].shape == (NB, 4, 6, N) and r["observed"].shape == (NB, 4, 6, P) and r["G"].shape == (NB, N, N)
    call(*_model(), np.zeros((NB, 4, 5, 1, K)), mode="news")
    assert (recorded.named["eps_batched"], recorded.named["n_lead"]) == (1, 0)
    for x0, flags in ((np.zeros(N), (0, 0)), (np.zeros((4, N)), (0, 1)), (np.zeros((NB, 1, N)), (1, 0)), (np.zeros((NB, 4, N)), (1, 1)),
                      (np.zeros((1, 4, N)), (0, 1)), (np.zeros((1, 1, N)), (0, 0))):
        call(*_model(), np.zeros((4, 7, K)), x0=x0)
        assert (recorded.named["x0_batched"], recorded.named["x0_paths"]) == flags, x0.shape
    status = np.array([0, 1], dtype=np.int32)
    r = call(*_model(), np.zeros((4, 7, K)), status=status)
    assert r["status"] is not status and r["status"].tolist() == [0, 1]  # (the in/out word is a copy)


def test_every_refusal_comes_before_anything_is_staged(no_library):
    call = batched.anticipated_paths_batched
    eps = np.zeros((4, 7, K))
    with pytest.raises(ValueError, match="at most 64"):
        call(*_model(n=65), eps)
    with pytest.raises(ValueError, match="n_lead = 64"):
        call(*_model(), np.zeros((1, 2, 65, K)), mode="news")
    with pytest.raises(ValueError, match="news needs at least"):
        call(*_model(), np.zeros((1, 5, 2, K)), mode="news", n_steps=4)
    with pytest.raises(ValueError, match="outputs must name"):
        call(*_model(), eps, outputs=())
    with pytest.raises(ValueError, match="outputs must name"):
        call(*_model(), eps, outputs=("x", "shocks"))
    with pytest.raises(ValueError, match="mode must be"):
        call(*_model(), eps, mode="foresight")
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), np.zeros((4, 7, K + 1)))
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), np.zeros((7, K)))
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), eps, mode="news")  # news needs the lead axis
    with pytest.raises(ValueError, match="eps must be"):
        call(*_model(), np.zeros((NB + 1, 4, 7, K)))
    B, C, T, R = _model()
    with pytest.raises(ValueError, match="B and C must be"):
        call(B[:1], C, T, R, eps)
    with pytest.raises(ValueError, match="B and C must be"):
        call(B, np.zeros((NB, N, N + 1)), T, R, eps)
    with pytest.raises(ValueError, match="x0 must be"):
        call(B, C, T, R, eps, x0=np.zeros((3, N)))
    with pytest.raises(ValueError, match="x0 must be"):
        call(B, C, T, R, eps, x0=np.zeros((NB, 4, N + 1)))
    with pytest.raises(ValueError, match="need Z"):
        call(B, C, T, R, eps, outputs=("observed",))
    with pytest.raises(ValueError, match="need Z"):
        call(B, C, T, R, eps, d=np.zeros(P))
    with pytest.raises(ValueError, match="Z must be"):
        call(B, C, T, R, eps, Z=np.eye(P, N + 1))
    with pytest.raises(ValueError, match="at most 16"):
        call(*_model(n=20), eps, Z=np.eye(17, 20))
    with pytest.raises(ValueError, match="status must be"):
        call(B, C, T, R, eps, status=np.zeros(NB + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="an output buffer"):
        from geconpy_amd import _frontend as F

        F.anticipated_paths(F.HOST, "anticipated_paths_batched", B, C, T, R, eps, n_steps=None, mode="perfect_foresight", x0=None,
                            Z=None, d=None, status=None, rank_tol=0.0, outputs=("x",), out=dict(x=np.empty((NB, 4, 6, N))))


def _raw(B, C, T, R, *, mode=0, n_lead=0, n_steps=5, n_shock=5, n_paths=1, p=0, Z=None, eps="zeros", outs=(True, False, False, False)):
    """The host twin called directly: the return code, with everything after the refusal never reached on a machine without a GPU."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nb, n, k = (NB, N, K) if R is None else R.shape
    eps = np.zeros((max(n_paths, 1), max(n_shock, 1) * (n_lead + 1 if n_lead > 0 else 1), k)) if isinstance(eps, str) else eps
    x, w, o, g = (np.empty(nb * max(n_paths, 1) * max(n_steps, 1) * max(n, 16)) if on else None for on in outs)
    return lib.dsge_anticipated_paths_batched_host(ptr(B), ptr(C), ptr(T), ptr(R), ptr(eps), 0, mode, n_lead, None, 0, 0, ptr(Z), 0, None,
                                                   0, None, nb, n, k, p, n_paths, n_steps, n_shock, 0.0, ptr(x), ptr(w), ptr(o), ptr(g))


def test_the_library_refuses_sizes_before_any_device():
    big, err = _lib.ERR_TOO_LARGE, lambda: _lib.load().dsge_last_error()  # noqa: E731
    assert _raw(*_model(n=65)) == big and b"DSGE_MAX_N" in err()
    assert _raw(*_model(n=96)) == big
    assert _raw(*_model(n=20), p=17, Z=np.eye(17, 20)) == big and b"DSGE_MAX_P" in err()
    assert _raw(*_model(), mode=1, n_lead=64) == big and b"n_lead" in err()
    # what is inside the limits is not refused: it goes on to the device
    assert _raw(*_model(n=64, k=32), p=16, Z=np.eye(16, 64)) in (0, _lib.ERR_HIP)
    assert _raw(*_model(), mode=1, n_lead=63) in (0, _lib.ERR_HIP)
    with pytest.raises(ValueError):
        batched.anticipated_paths_batched(*_model(n=65), np.zeros((1, 2, K)))


def test_the_library_refuses_malformed_calls_before_any_device():
    bad, err = _lib.ERR_INVALID, lambda: _lib.load().dsge_last_error()  # noqa: E731
    B, C, T, R = _model()
    assert _raw(B, C, T, R, mode=2) == bad and b"mode" in err()
    assert _raw(B, C, T, R, mode=-1) == bad
    assert _raw(B, C, T, R, mode=1, n_lead=-1) == bad and b"n_lead" in err()
    assert _raw(B, C, T, R, mode=0, n_lead=1) == bad and b"perfect foresight" in err()
    assert _raw(B, C, T, R, mode=1, n_steps=4, n_shock=5) == bad and b"n_shock_steps > n_steps" in err()
    assert _raw(B, C, T, R, mode=0, n_steps=1, n_shock=4) in (0, _lib.ERR_HIP)  # perfect foresight: shocks beyond the horizon
    assert _raw(None, C, T, R) == bad and _raw(B, None, T, R) == bad and _raw(B, C, None, R) == bad and _raw(B, C, T, None) == bad
    assert _raw(B, C, T, R, eps=None) == bad and b"null pointer" in err()
    assert _raw(B, C, T, R, eps=None, n_shock=0) in (0, _lib.ERR_HIP)  # no shock at all needs no eps
    assert _raw(B, C, T, R, outs=(False, False, False, False)) == bad and b"no output" in err()
    assert _raw(B, C, T, R, outs=(False, False, False, True)) in (0, _lib.ERR_HIP)  # G alone is an output
    assert _raw(B, C, T, R, outs=(False, False, True, False)) == bad and b"p == 0" in err()  # observed without Z
    assert _raw(B, C, T, R, p=2) == bad and b"without Z" in err()
    assert _raw(*_model(n=3, k=4)) == bad
    assert _raw(B, C, T, R, n_steps=-1) == bad and _raw(B, C, T, R, n_paths=-1) == bad


def test_abi_version_and_status_constant_match_the_header():
    assert _lib.ABI_VERSION >= 17
    text = open(os.path.join(ROOT, "include", "dsge_hip.h")).read()
    consts = dict(re.findall(r"#define\s+(DSGE_[A-Z_0-9]+)\s+(-?\d+)", text))
    assert int(consts["DSGE_ST_ANTICIPATION_SINGULAR"]) == _lib.ST_ANTICIPATION_SINGULAR == 2048
    assert int(consts["DSGE_ANT_PERFECT_FORESIGHT"]) == _lib.ANT_PERFECT_FORESIGHT
    assert int(consts["DSGE_ANT_NEWS"]) == _lib.ANT_NEWS
    assert int(consts["DSGE_ANT_MAX_LEAD"]) == _lib.ANT_MAX_LEAD == 63
    assert int(consts["DSGE_ABI_VERSION"]) == _lib.ABI_VERSION
    sig = [name for name, _ in _lib.SIGNATURES["dsge_anticipated_paths_batched"]]
    assert sig[-1] == "stream" and [name for name, _ in _lib.SIGNATURES["dsge_anticipated_paths_batched_host"]] == sig[:-1]


def test_no_kernel_of_the_entry_spills_to_scratch_memory(tmp_path):
    """The setup kernel keeps sixteen entries of M per thread in registers, the paths kernel a slab and up to four shock rows in
    flight; a compiler that starts to spill them must not go unnoticed."""
    import subprocess

    from geconpy_amd import build

    out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "a.o"),
                          os.path.join(build.CSRC, "launch_anticipated.hip")], cwd=build.CSRC, capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S*ant_\S*kernel\S*)", out.stderr)
    sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len({n for n in names if "setup" in n}) == 1 and len({n for n in names if "paths" in n}) == 2
    assert len(sizes) >= 3 and set(sizes) == {"0"}
