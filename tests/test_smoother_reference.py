"""CPU: the numpy restatement of the smoother recursion (tests/smoother_reference.py) against brute-force conditioning of the
joint Gaussian, and the shape checks of the smoother's numpy wrapper (no GPU needed: they run before anything is staged)."""
import numpy as np
import pytest

import oracle
from oracle.cycle_reduction import cycle_reduction_core
from geconpy_amd import batched
from geconpy_amd import workloads as wl

from tests import smoother_cases as cases
from tests.smoother_reference import brute_force_smoother, range_smoother, rts_smoother


@pytest.mark.parametrize("model", ["rbc", "full_nk"])
def test_rts_recursion_matches_joint_gaussian_conditioning(model):
    """8 steps, two observables (one state, one non-state variable), H = 1e-6 I, one partial-missing and one empty row, filter
    without the P jitter and the Joseph form -- then the stored filter IS the exact filter of the model with noise H + jitter_F,
    and the pinv recursion (states, covariances, shocks from t >= 1) must reproduce the conditional moments to 1e-9 relative
    (measured: 6e-11 RBC, 3e-13 full_nk)."""
    b, _ = (wl.rbc_batch if model == "rbc" else wl.full_nk_batch)(1)
    A, B, C, D = (b[x][0] for x in "ABCD")
    T, ok, _ = cycle_reduction_core(A, B, C, 1000, 1e-12)
    assert ok
    R = oracle.compute_selection_matrix(B, C, D, T)
    m = T.shape[0]
    is_state = np.abs(T).sum(axis=0) > 0
    Z = np.zeros((2, m))
    Z[0, np.flatnonzero(is_state)[0]] = 1.0
    Z[1, np.flatnonzero(~is_state)[0]] = 1.0
    Q = np.diag(b["sigma"][0] ** 2)
    y = np.random.default_rng(3).normal(0, 0.02, (8, 2))
    y[3, 1] = np.nan
    y[5] = np.nan
    H = 1e-6 * np.eye(2)
    cv = oracle.FilterConventions(jitter_on_P=False, joseph=False)
    _, _, stt = oracle.kalman_filter_logp(y, T, R, Q, Z, H=H, return_states=True, conventions=cv)
    a, V, e = rts_smoother(stt, T, R, Q)
    a2, V2, e2 = brute_force_smoother(y, T, R, Q, Z, H, oracle.JITTER_DEFAULT)
    assert np.isnan(e[0]).all()
    errs = (np.abs(a - a2).max() / np.abs(a2).max(), np.abs(V - V2).max() / np.abs(V2).max(),
            np.abs(e[1:] - e2[1:]).max() / np.abs(e2[1:]).max())
    print(model, errs)
    assert max(errs) <= 1e-9, errs
    assert np.abs(a - stt["a_filt"]).max() > 1e-2 * np.abs(a2).max()  # (smoothing is not trivially the filter)


@pytest.mark.parametrize("name", cases.ALL_CASES)
def test_range_form_matches_pinv_form(name):
    """The condition on the INPUTS of every edge case the device is held to (tests/smoother_cases.py): the device's form of the
    recursion, restated in numpy (range_smoother: U M^-1 U' on the range of [T | R_J]), and the reference's (rts_smoother:
    pinv(hermitian=True)) agree within 1e-10 x scale on states, covariances and shocks -- one decade under the device's bar, so
    that the reference's own noise cannot decide a device test --, the range has the expected dimension, and smoothing moves the
    states by at least 1e-3 x scale.  (Measured: <= 1.5e-13 on the zero-column models, <= 8e-13 on the dense ones, 2e-12 without the F jitter.)"""
    c = cases.case(name)
    for i, (_, stt, a, V, e) in cases.reference(name).items():
        x = cases.draw(c, i)
        a2, V2, e2, r, lam = range_smoother(stt, x["T"], x["R"], x["Q"])
        sc, pc, ec = cases.scales(c, i, stt)
        errs = (np.abs(a2 - a).max() / sc, np.abs(V2 - V).max() / pc, np.abs(e2[1:] - e[1:]).max() / ec)
        print(name, i, "r =", r, "lambda_min/lambda_max(M) =", lam, "range form - pinv form / scale (states, covs, shocks):", errs)
        assert r == c["r"]
        assert np.isnan(e[0]).all() and np.isnan(e2[0]).all()
        assert max(errs) <= 1e-10, errs
        assert np.abs(a - stt["a_filt"]).max() / sc >= 1e-3
        if c.get("zero_shock") is not None:
            assert (e[1:, c["zero_shock"]] == 0.0).all() and (e2[1:, c["zero_shock"]] == 0.0).all()


def test_smoother_wrapper_shape_checks():
    T = np.zeros((2, 4, 4))
    R = np.zeros((2, 4, 1))
    y = np.zeros((5, 1))
    Z = np.zeros((1, 4))
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T[:, :3], R, np.ones(1), Z, y)
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, np.zeros((2, 3, 1)), np.ones(1), Z, y)
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, R, np.ones(1), np.zeros((2, 3)), y)
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, R, np.ones(3), Z, y, q_mode="diag")
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, R, np.ones(1), Z, y, Hdiag=np.zeros(2))
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(np.zeros((1, 65, 65)), np.zeros((1, 65, 1)), np.ones(1), np.zeros((1, 65)), y)
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, R, np.ones(1), Z, y, scratch_limit_bytes=-1)
    with pytest.raises(ValueError):
        batched.kalman_smoother_batched(T, R, np.ones(1), Z, y, status=np.zeros(3, dtype=np.int32))
    assert batched.smoother_scratch_bytes_per_draw(40, 200) == 8 * (2 * 200 * 1600 + 2 * 200 * 40)
