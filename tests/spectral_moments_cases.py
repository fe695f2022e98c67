"""Inputs of the spectral-moments tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): models, covariances, design
matrices and gains, built once, read-only, with the numpy reference of every case computed once.  Shared by
tests/test_spectral_moments_reference.py (CPU) and tests/test_gpu_spectral_moments.py."""
import functools

import numpy as np

from geconpy_amd import batched
from tests import spectral_moments_reference as ref
from tests.shock_decomposition_cases import model

NB = 3
COND_BOUND = 1e5


def _q(name, k, mode):
    rng = np.random.default_rng([53, k, len(name)])
    if mode == "diag":
        return rng.uniform(0.5, 1.5, k) * 1e-2
    if mode == "diag_batched":
        return rng.uniform(0.5, 1.5, (NB, k)) * 1e-2
    L = rng.standard_normal((NB, k, k)) * 0.1
    Qf = L @ L.transpose(0, 2, 1) + 1e-2 * np.eye(k)
    return Qf[0].copy() if mode == "full" else Qf


def _selector(m, rows):
    Z = np.zeros((len(rows), m))
    Z[np.arange(len(rows)), rows] = 1.0
    return Z


def _dense_z(name, p, m, batched_z):
    rng = np.random.default_rng([59, p, m])
    return rng.standard_normal((NB, p, m) if batched_z else (p, m)) / np.sqrt(m)


def unit_root_model():
    """``sw16`` plus one cumulator row: x_c[t] = x_c[t-1] + x_0[t], an exact root 1 of T (its column of I - T is exactly zero)."""
    T0, R0 = model("sw16")
    nb, m, k = R0.shape
    T, R = np.zeros((nb, m + 1, m + 1)), np.zeros((nb, m + 1, k))
    T[:, :m, :m], R[:, :m] = T0, R0
    T[:, m, :m], T[:, m, m], R[:, m] = T0[:, 0], 1.0, R0[:, 0]
    return T, R


# name -> (model, n_grid, n_lags, q_mode, Z, Hdiag, gain, correlation, spectrum, acov); Z: None, ("sel", rows), ("dense", p, batched)
_SPEC = {
    "rbc": ("rbc", 8, 4, "diag", None, None, None, False, False, True),
    "sw16_hp": ("sw16", 64, 4, "diag_batched", ("sel", (0, 3, 7)), "shared", "hp", True, False, True),
    "sw17_band": ("sw17", 66, 5, "full", ("dense", 4, False), "batched", "band", False, True, True),
    "wide33_16": ("wide33_16", 64, 3, "full_batched", None, None, None, True, False, True),
    "wide40_32": ("wide40_32", 16, 2, "diag", None, None, "hp", False, False, True),
    "sw40_hp": ("sw40", 256, 10, "diag", ("sel", (0, 1, 2, 3, 4, 5, 6)), None, "hp", False, False, True),
    "sw40_hp_states": ("sw40", 256, 2, "diag", None, None, "hp", False, False, True),
    "sw49_dense": ("sw49", 64, 0, "diag_batched", ("dense", 5, True), None, None, False, True, False),
    "sw64": ("sw64", 32, 1, "full", None, None, None, False, False, True),
    "nk_persistent": ("full_nk", 1024, 8, "diag", ("sel", (0, 5, 11)), "shared", None, True, False, True),
    "sw17_unit_root": ("unit_root", 64, 4, "diag", ("sel", (0, 2, 16)), None, "hp", False, False, True),
}
NAMES = tuple(_SPEC)


@functools.lru_cache(maxsize=None)
def case(name):
    """The keyword arguments of ``batched.spectral_moments_batched`` for the case (arrays read-only)."""
    mdl, n_grid, n_lags, q_mode, z, h, gain, corr, spectrum, acov = _SPEC[name]
    T, R = unit_root_model() if mdl == "unit_root" else model(mdl, NB)
    m, k = R.shape[1:]
    Z = None if z is None else (_selector(m, z[1]) if z[0] == "sel" else _dense_z(name, z[1], m, z[2]))
    p = 0 if Z is None else Z.shape[-2]
    Hdiag = None if h is None else np.random.default_rng([61, p]).uniform(1e-4, 1e-3, (NB, p) if h == "batched" else (p,))
    g = None if gain is None else (batched.hp_gain(n_grid) if gain == "hp" else batched.bandpass_gain(n_grid))
    kw = dict(T=T, R=R, Q=_q(name, k, q_mode), n_grid=n_grid, n_lags=n_lags, Z=Z, Hdiag=Hdiag, gain=g, correlation=corr,
              spectrum=spectrum, q_mode=q_mode, acov=acov)
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy reference of the case (computed once, read-only): dict(acov, spectrum, cond)."""
    kw = dict(case(name))
    kw.pop("acov")
    r = ref.spectral_moments(kw.pop("T"), kw.pop("R"), kw.pop("Q"), kw.pop("q_mode"), kw.pop("n_grid"), kw.pop("n_lags"), **kw)
    for v in r.values():
        v.setflags(write=False)
    return r
