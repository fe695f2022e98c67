"""CPU: the front end of the spectral moments (``_frontend.spectral_moments``) refuses what is malformed before any call, the
library refuses what is too large or malformed before any device is touched (this machine may have none), and the two gain
helpers return what they say."""
import os
import re

import numpy as np
import pytest

from geconpy_amd import _lib, batched

NB, M, K, P, N = 2, 6, 3, 2, 16


def _inputs(nb=NB, m=M, k=K):
    return np.zeros((nb, m, m)), np.zeros((nb, m, k)), np.ones(k)


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _NoCall())


class _Recorder:
    def __call__(self, entry, *, host, stream=None, **named):
        self.entry, self.named = entry, named


@pytest.fixture
def recorded(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def test_abi_version_and_status_constant_match_the_header():
    assert _lib.ABI_VERSION >= 16
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "dsge_hip.h")) as fh:
        consts = dict(re.findall(r"#define\s+(DSGE_[A-Z_0-9]+)\s+(-?\d+)", fh.read()))
    assert int(consts["DSGE_ST_SPECTRAL_SINGULAR"]) == _lib.ST_SPECTRAL_SINGULAR == 1024
    assert int(consts["DSGE_ABI_VERSION"]) == _lib.ABI_VERSION


def test_hp_gain():
    g = batched.hp_gain(512)
    assert g.shape == (257,) and g[0] == 0.0 and np.all(np.diff(g) > 0.0) and g[-1] < 1.0
    w = 2.0 * np.pi * 40 / 512
    c = 4.0 * 1600.0 * (1.0 - np.cos(w)) ** 2
    assert g[40] == pytest.approx((c / (1.0 + c)) ** 2, rel=1e-15)
    assert batched.hp_gain(512, lam=100.0)[40] < g[40]


def test_bandpass_gain_edges():
    g = batched.bandpass_gain(96)  # 2 pi / 32 = w_3 and 2 pi / 6 = w_16 are grid points: both edges belong to the band
    assert g.shape == (49,) and g.tolist() == [0.0] * 3 + [1.0] * 14 + [0.0] * 32
    g = batched.bandpass_gain(64, low=8, high=16)
    assert np.flatnonzero(g).tolist() == [4, 5, 6, 7, 8]
    assert batched.bandpass_gain(66).sum() == 9  # n = 3 .. 11
    for n_grid in range(4, 4097, 2):  # an edge that is a grid point belongs to the band, whatever 2 pi n / N rounds to
        for low, high in ((6, 32), (2, 8), (3, 7)):
            g = batched.bandpass_gain(n_grid, low=low, high=high)
            inside = [n for n in range(n_grid // 2 + 1) if n * high >= n_grid and n * low <= n_grid]
            assert np.flatnonzero(g).tolist() == inside
            if n_grid % high == 0:
                assert g[n_grid // high] == 1.0 and g[n_grid // high - 1] == 0.0
            if n_grid % low == 0:
                assert g[n_grid // low] == 1.0 and (n_grid // low == n_grid // 2 or g[n_grid // low + 1] == 0.0)
    with pytest.raises(ValueError):
        batched.bandpass_gain(64, low=32, high=6)
    with pytest.raises(ValueError):
        batched.hp_gain(63)


def test_shape_and_argument_errors_are_value_errors(no_library):
    T, R, Q = _inputs()
    call = batched.spectral_moments_batched
    for bad in (15, 2, 4098):
        with pytest.raises(ValueError, match="n_grid"):
            call(T, R, Q, n_grid=bad)
    with pytest.raises(ValueError, match="n_lags"):
        call(T, R, Q, n_grid=N, n_lags=N // 2 + 1)
    with pytest.raises(ValueError, match="n_lags"):
        call(T, R, Q, n_grid=N, n_lags=-1)
    with pytest.raises(ValueError, match="Hdiag"):
        call(T, R, Q, n_grid=N, n_lags=2, Hdiag=np.ones(P))
    with pytest.raises(ValueError, match="Z must be"):
        call(T, R, Q, n_grid=N, n_lags=2, Z=np.eye(P, M + 1))
    with pytest.raises(ValueError, match="Hdiag"):
        call(T, R, Q, n_grid=N, n_lags=2, Z=np.eye(P, M), Hdiag=np.ones(P + 1))
    with pytest.raises(ValueError, match="gain"):
        call(T, R, Q, n_grid=N, n_lags=2, gain=np.ones(N // 2))
    with pytest.raises(ValueError, match="status"):
        call(T, R, Q, n_grid=N, n_lags=2, status=np.zeros(NB + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="Q"):
        call(T, R, np.ones(K + 1), n_grid=N, n_lags=2)
    with pytest.raises(ValueError, match="nothing to compute"):
        call(T, R, Q, n_grid=N, n_lags=2, acov=False)
    with pytest.raises(ValueError, match="scratch_limit_bytes"):
        call(T, R, Q, n_grid=N, n_lags=2, scratch_limit_bytes=-1)
    with pytest.raises(ValueError, match="T must be"):
        call(T, np.zeros((NB, M + 1, K)), Q, n_grid=N, n_lags=2)


def test_shapes_become_the_arguments_of_the_abi(recorded):
    T, R, Q = _inputs()
    r = batched.spectral_moments_batched(T, R, Q, n_grid=N, n_lags=3, Z=np.zeros((NB, P, M)), Hdiag=np.ones(P), spectrum=True,
                                         gain=batched.hp_gain(N), correlation=True)
    a = recorded.named
    assert recorded.entry == "dsge_spectral_moments_batched"
    assert (a["batch"], a["m"], a["k"], a["p"], a["n_grid"], a["n_lags"], a["z_batched"], a["h_batched"], a["correlation"]) == \
        (NB, M, K, P, N, 3, 1, 0, 1)
    assert a["q_mode"] == _lib.Q_DIAG_SHARED and a["rank_tol"] == 0.0 and a["scratch_limit_bytes"] == 0
    assert r["acov"].shape == (NB, 4, P, P) and r["spectrum"].shape == (NB, N // 2 + 1, P, P) and r["spectrum"].dtype == np.complex128
    assert r["freqs"].shape == (N // 2 + 1,) and r["freqs"][-1] == pytest.approx(np.pi) and r["status"].dtype == np.int32
    r = batched.spectral_moments_batched(T, R, Q, n_grid=N, n_lags=0)
    a = recorded.named
    assert a["Z"] is None and a["p"] == 0 and a["spectrum_out"] is None and a["gain"] is None and r["acov"].shape == (NB, 1, M, M)
    assert "spectrum" not in r


def _raw(nb=1, m=M, k=K, p=P, n_grid=N, n_lags=2, z=True, h=False, acov=True, spec=False, missing=()):
    """The host twin with raw arguments; -> the return code of the refusal (the call must not reach a device)."""
    T, R, Q = _inputs(nb, m, k)
    dim = p if z else m
    bufs = dict(T=T, R=R, Q=Q, Z=np.zeros((max(p, 1), m)) if z else None, Hdiag=np.ones(max(p, 1)) if h else None, gain=None,
                acov_out=np.empty((nb, max(n_lags, 0) + 1, max(dim, 1), max(dim, 1))) if acov else None,
                spectrum_out=np.empty((nb, max(n_grid, 2) // 2 + 1, max(dim, 1), max(dim, 1)), dtype=np.complex128) if spec else None,
                status_io=np.zeros(nb, dtype=np.int32))
    for name in missing:
        bufs[name] = None
    with pytest.raises(_lib.DsgeHipError) as err:
        _lib.call("dsge_spectral_moments_batched", host=True, q_mode=_lib.Q_DIAG_SHARED, z_batched=0, h_batched=0, batch=nb, m=m, k=k,
                  p=p, n_grid=n_grid, n_lags=n_lags, correlation=0, rank_tol=0.0, scratch_limit_bytes=0,
                  **{key: None if v is None else v.ctypes.data for key, v in bufs.items()})
    return err.value


@pytest.mark.parametrize("over", [dict(n_grid=15), dict(n_grid=2), dict(n_grid=4098), dict(n_lags=-1), dict(n_lags=N // 2 + 1),
                                  dict(z=False, h=True), dict(missing=("T",)), dict(missing=("R",)), dict(missing=("Q",)),
                                  dict(k=0), dict(k=M + 1), dict(p=0), dict(acov=False, spec=False)])
def test_malformed_calls_are_refused_before_any_device_is_touched(over):
    err = _raw(**over)
    assert err.code == _lib.ERR_INVALID and not isinstance(err, _lib.DsgeTooLargeError)


@pytest.mark.parametrize("over", [dict(m=65, k=4), dict(m=40, k=33), dict(p=65), dict(m=64, k=32, p=64), dict(m=64, k=32, p=46)])
def test_sizes_beyond_the_limits_are_too_large(over):
    err = _raw(**over)
    assert err.code == _lib.ERR_TOO_LARGE and isinstance(err, _lib.DsgeTooLargeError)


def test_no_instance_of_the_solve_kernel_spills_to_scratch_memory(tmp_path):
    """The elimination keeps a row of up to 96 complex entries in registers; a compiler that stops doing so must not go unnoticed."""
    import subprocess

    from geconpy_amd import build

    out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "s.o"),
                          os.path.join(build.CSRC, "launch_spectral.hip")], cwd=build.CSRC, capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S*spectral\S*)", out.stderr)
    sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len({n for n in names if "solve" in n}) == 6 and len({n for n in names if "reduce" in n}) == 1
    assert len(sizes) >= 7 and set(sizes) == {"0"}
