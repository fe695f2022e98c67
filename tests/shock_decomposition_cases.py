"""Inputs of the shock-decomposition tests (TEST INFRASTRUCTURE ONLY; a helper, not a test module): models and paths, built once,
read-only, shared by tests/test_shock_decomposition_reference.py (CPU) and tests/test_gpu_shock_decomposition.py."""
import functools

import numpy as np

import oracle
from geconpy_amd import workloads as wl

SW = {"sw16": dict(n=16, n_state=7, n_lead=5, k=3), "sw17": dict(n=17, n_state=7, n_lead=5, k=3), "sw40": {},
      "sw49": dict(n=49, n_state=22, n_lead=15, k=7), "sw64": dict(n=64, n_state=30, n_lead=20, k=8),
      "sw96": dict(n=96, n_state=40, n_lead=30, k=8)}


def _selection(b, T):
    return np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(T.shape[0])])


@functools.lru_cache(maxsize=None)
def model(name, nb=3):
    """(T (nb, m, m), R (nb, m, k)), every draw distinct: "rbc" (m = 8, k = 1), "full_nk" (24, 4), the SW-shaped ``SW`` and
    "wide<m>_<k>": a stable dense T with k shocks (for k = 15 and 16, which no model of the package has)."""
    if name in ("rbc", "full_nk"):
        b, _ = (wl.rbc_batch if name == "rbc" else wl.full_nk_batch)(nb)
        T = np.empty_like(b["A"])
        for i in range(nb):
            T[i], ok, _ = oracle.cycle_reduction.cycle_reduction_core(b["A"][i], b["B"][i], b["C"][i], 1000, 1e-12)
            assert ok
        R = _selection(b, T)
    elif name.startswith("wide"):
        m, k = (int(v) for v in name[4:].split("_"))
        rng = np.random.default_rng([41, m, k])
        T = np.stack([0.7 * np.linalg.qr(rng.standard_normal((m, m)))[0] + 0.1 * rng.standard_normal((m, m)) / np.sqrt(m)
                      for _ in range(nb)])
        assert max(np.abs(np.linalg.eigvals(t)).max() for t in T) < 0.95
        R = rng.standard_normal((nb, m, k)) / np.sqrt(m)
    else:
        b = wl.sw_shaped_batch(nb, **SW[name])
        T = np.ascontiguousarray(b["T_star"])
        R = _selection(b, T)
    T, R = np.ascontiguousarray(T), np.ascontiguousarray(R)
    T.setflags(write=False)
    R.setflags(write=False)
    return T, R


def shocks(nb, n_paths, T_len, k, seed=0):
    """(nb, n_paths, T_len, k) ~ 0.01 N(0, 1) with period 0 NaN, as the smoother writes them."""
    e = 0.01 * np.random.default_rng([7, seed]).standard_normal((nb, n_paths, T_len, k))
    e[:, :, 0] = np.nan
    return e


def exact_paths(T, R, e, seed=0):
    """(nb, n_paths, T_len, m): x[0] ~ 0.05 N(0, 1), x[t] = T x[t-1] + R e[t] -- the states are about 0.05, as smoothed ones are."""
    nb, n_paths, T_len, _ = e.shape
    m = T.shape[1]
    x = np.empty((nb, n_paths, T_len, m))
    x[:, :, 0] = 0.05 * np.random.default_rng([8, seed]).standard_normal((nb, n_paths, m))
    for t in range(1, T_len):
        x[:, :, t] = np.einsum("bij,bsj->bsi", T, x[:, :, t - 1]) + np.einsum("bij,bsj->bsi", R, e[:, :, t])
    return x
