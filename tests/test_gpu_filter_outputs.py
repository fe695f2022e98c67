"""GPU: the per-step outputs kernel (kalman_filter_outputs_batched, csrc/dsge_kalman_out.hpp) against the oracle's recursion
(oracle.kalman_filter_logp(..., return_states=True)) at the sizes tests/test_gpu_parity.py::test_kalman_filter_outputs_per_step
(m = 40, p = 7, diagonal Q, shared Z) does not reach: m = 1, 17, 40, 64; p = 1, 4, 9 and 16 = KO_PMAX (tid < p * p takes all 256
threads, x[PM] and the one-thread Cholesky run at full width); a full Q, shared and per draw; Z, d and Hdiag per draw.

Bars: those of that test -- 1e-9 x scale on states and covariances (sc = max(1, |a_filt|max), pc = |P_pred|max), ll at
rtol = 1e-8, atol = 1e-9, and the per-step ll sums to kalman_logp_batched at rtol = 1e-10."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import oracle
from geconpy_amd import batched

from tests import smoother_cases as cases

pytestmark = pytest.mark.gpu

N_STEPS = 10
# (m, p) -> the zero-column shape (n, n_state, n_lead, k) of the model; m = 1 is the dense recipe (k = 1)
SIZES = {(1, 1): None, (17, 1): (17, 7, 5, 3), (17, 9): (17, 7, 5, 3), (40, 16): (40, 18, 12, 7), (64, 16): (64, 30, 20, 8),
         (64, 4): (64, 30, 20, 8)}
VARIANTS = ("shared", "per_draw")


def _partial_missing(p):
    """The entries left out of the partial-missing row: 3 and 15 at p = 16."""
    return [3, p - 1] if p >= 5 else [2] if p >= 3 else []


@functools.lru_cache(maxsize=None)
def _inputs(m, p, variant):
    """"shared": one full Q, one Z, no d, one Hdiag for the 2 draws; "per_draw": a full Q, Z, d and Hdiag per draw, all different.
    10 steps simulated from draw 0; row 3 partially missing (p >= 3), row 6 empty."""
    rng = np.random.default_rng([23, m, p, VARIANTS.index(variant)])
    nb = 2
    if SIZES[(m, p)] is None:
        T, R, sigma, _ = cases.dense_model(nb, m, 1, p, rng)
    else:
        T, R, sigma = cases.sw_model(nb, SIZES[(m, p)])
    Z = rng.standard_normal((p, m)) * (rng.random((p, m)) < 0.3)
    Z[np.arange(p), np.arange(p) % m] = 1.0
    H = np.full(p, 1e-4)
    Ls = [cases.chol_factor(sigma[i], rng) for i in range(nb)]
    if variant == "shared":
        c = dict(T=T, R=R, q=Ls[0] @ Ls[0].T, q_mode="full", Z=Z, d=None, H=H)
    else:
        scale = 1.0 + np.arange(nb) / 8.0
        Zb = Z[None] * scale[:, None, None] + 0.05 * rng.standard_normal((nb, p, m)) * (Z != 0)
        c = dict(T=T, R=R, q=np.stack([L @ L.T for L in Ls]), q_mode="full_batched", Z=Zb, d=rng.normal(0, 0.01, (nb, p)),
                 H=H[None] * scale[:, None] ** 2)
    y = cases.simulate(c, N_STEPS, rng)
    y[3, _partial_missing(p)] = np.nan
    y[6] = np.nan
    c["y"] = y
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m,p", list(SIZES))
def test_outputs_against_the_oracle(m, p, variant):
    c = _inputs(m, p, variant)
    kw = dict(d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"])
    out = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], full_covariances=True, **kw)
    diag = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], **kw)
    lp, st = batched.kalman_logp_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], **kw)
    assert (out["status"] == 0).all() and (diag["status"] == 0).all() and (st == 0).all()
    assert_allclose(out["ll"].sum(axis=1), lp, rtol=1e-10)
    assert_array_equal(out["ll"], diag["ll"])
    for i in range(c["T"].shape[0]):
        x = cases.draw(c, i)
        _, ll, stt = oracle.kalman_filter_logp(c["y"], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], return_states=True)
        sc, pc = max(1.0, np.abs(stt["a_filt"]).max()), np.abs(stt["P_pred"]).max()
        errs = {k_: np.abs(out[k_][i] - stt[r_]).max() / s_ for k_, r_, s_ in (
            ("predicted_states", "a_pred", sc), ("filtered_states", "a_filt", sc), ("predicted_covs", "P_pred", pc),
            ("filtered_covs", "P_filt", pc))}
        print((m, p), variant, i, "errors / scale:", errs, "ll:", np.abs(out["ll"][i] - ll).max())
        assert_allclose(out["ll"][i], ll, rtol=1e-8, atol=1e-9)
        assert ll[6] == 0.0 and out["ll"][i, 6] == 0.0
        assert_allclose(out["predicted_states"][i], stt["a_pred"], rtol=0, atol=1e-9 * sc)
        assert_allclose(out["filtered_states"][i], stt["a_filt"], rtol=0, atol=1e-9 * sc)
        assert_allclose(out["predicted_covs"][i], stt["P_pred"], rtol=0, atol=1e-9 * pc)
        assert_allclose(out["filtered_covs"][i], stt["P_filt"], rtol=0, atol=1e-9 * pc)
        assert_allclose(diag["predicted_states"][i], stt["a_pred"], rtol=0, atol=1e-9 * sc)
        assert_allclose(diag["filtered_states"][i], stt["a_filt"], rtol=0, atol=1e-9 * sc)
        assert_allclose(diag["predicted_covs"][i], np.diagonal(stt["P_pred"], axis1=1, axis2=2), rtol=0, atol=1e-9 * pc)
        assert_allclose(diag["filtered_covs"][i], np.diagonal(stt["P_filt"], axis1=1, axis2=2), rtol=0, atol=1e-9 * pc)
