"""GPU: the device front-end (``LogpEngine``) and the numpy front-end (``batched``) are one body over two backends, so with the same
explicit hints and options both take the same kernel route and return the same bits -- here for the two paired entries no other
test compares: the gradient (selector and dense Z) and second order."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import batched
from geconpy_amd import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from geconpy_amd.engine import LogpEngine

    return LogpEngine(0)


@pytest.mark.parametrize("dense_z", [False, True])
def test_gradient_engine_equals_host_twin(eng, dense_z):
    """Every returned cotangent, logp and status of the RBC batch of test_gpu_gradient.py::test_gradient_rbc (6 draws, 10 steps)."""
    import torch

    rng = np.random.default_rng(0)
    th = wl.rbc_prior_draws(6, seed=4)
    A, B, C, D = wl.rbc_linearized_jacobians(**th)
    q = (th["sigma_A"] ** 2)[:, None]
    Z = np.zeros((2, 8))
    Z[0, wl.RBC_VARIABLES.index("Y")] = 1.0
    Z[1, wl.RBC_VARIABLES.index("C")] = 0.5
    y = rng.normal(0, 0.05, (10, 2))
    y[7, 0] = np.nan
    d, h = np.array([0.01, -0.02]), np.array([1e-4, 2e-4])
    state = np.any(A.reshape(-1, 8) != 0, axis=0)
    hint = int(np.count_nonzero(state if dense_z else state | np.any(Z != 0, axis=0)))  # (the rule of the numpy front-end)
    kw = dict(tol=1e-13, max_iter=200, n_filter_hint=hint, n_lead_hint=0, dense_z=dense_z, options={"kalman_grad_split": 2})
    ref = batched.solve_kalman_logp_grad_batched(A, B, C, D, q, Z, y, d=d, Hdiag=h, return_Z_bar=dense_z, **kw)
    assert np.all(ref["status"] == 0) and np.isfinite(ref["logp"]).all()
    dev = eng.to_device
    got = eng.solve_kalman_logp_grad(*(dev(x) for x in (A, B, C, D, q, Z, y)), d=dev(d), Hdiag=dev(h), **kw)
    torch.cuda.synchronize()
    keys = ["logp", "status", "A_bar", "B_bar", "C_bar", "D_bar", "q_bar", "d_bar", "h_bar"] + (["Z_bar"] if dense_z else [])
    assert sorted(got) == sorted(ref) == sorted(keys)
    for key in keys:
        assert_array_equal(got[key].cpu().numpy(), ref[key], err_msg=key)


def test_second_order_engine_equals_host_twin(eng):
    """logp and status of the smallest system of test_gpu_second_order.py::test_second_order_small_models (5 draws, 10 steps)."""
    import torch

    n, ns, nl, k, obs, nb = 6, 3, 2, 2, (0, 4, 5), 5
    sysm = [wl.sw_shaped_system(3100 + n + i, n=n, n_state=ns, n_lead=nl, k=k) for i in range(nb)]
    A, B, C, D = (np.stack([s_[j] for s_ in sysm]) for j in range(4))
    idx = wl.second_order_hessian_pattern(A[0], C[0], k, nnz_per_eq=6, seed=3100 + n)
    val = np.random.default_rng(3100 + n + 99).standard_normal((nb, len(idx)))
    rng = np.random.default_rng(n)
    q = rng.uniform(0.5e-4, 4e-4, (nb, k))
    Z = np.zeros((len(obs), n))
    Z[np.arange(len(obs)), list(obs)] = 1.0
    y = rng.normal(0, 0.02, (10, len(obs)))
    y[7, 0] = np.nan
    H, d = np.full(len(obs), 1e-5), rng.normal(0, 0.01, len(obs))
    structure = batched.second_order_structure(A, C, Z)
    kw = dict(tol=1e-12, max_iter=1000, options={"kalman_order": 1})
    ref = batched.second_order_logp_batched(A, B, C, D, idx, val, q, Z, y, d=d, Hdiag=H, structure=structure, **kw)
    assert (ref["status"] == 0).all() and np.isfinite(ref["logp"]).all()
    dev = eng.to_device
    d_idx = dev(np.asarray(idx, dtype=np.int32), torch.int32)
    logp, status = eng.second_order_logp(dev(A), dev(B), dev(C), dev(D), d_idx, dev(val), dev(q), dev(Z), dev(y), structure, d=dev(d),
                                         Hdiag=dev(H), **kw)
    torch.cuda.synchronize()
    assert_array_equal(logp.cpu().numpy(), ref["logp"])
    assert_array_equal(status.cpu().numpy(), ref["status"])
