"""Autograd reference of logp and its gradient (TEST INFRASTRUCTURE ONLY; a helper, not a test module): a plain torch float64 CPU
restatement of ``oracle.solve_kalman_logp`` -- A, B, C, D -> T -> R -> P0 -> filter -- differentiated by torch.autograd, so that
every ENTRY of every cotangent of the device's hand-derived reverse sweep has an independent value to be held to
(tests/test_gpu_gradient_entries.py; tests/test_gradient_reference.py holds this module to the oracle and to itself).
It shares no code with ``oracle.shared.policy_function_adjoints`` or with the device.  Every tensor lives on the CPU.

Two formulations of the part of the chain that is not a plain loop:

  "newton"    T* from ``oracle.cycle_reduction_core(A, B, C, 300, 1e-15)`` is a CONSTANT; one differentiable Newton step on
              F(T) = A + B T + C T^2 is applied to it, T = T* - L^-1 vec(A + B T* + C T*^2) with L = dF/dT at T* (detached:
              M (x) I + C (x) T*' on the row-major vec, M = B + C T*).  The value moves by the residual's rounding; the derivative of
              the step with respect to A, B, C is -L^-1 d(vec F): the implicit-function derivative exactly.
              P0 by the Kronecker solve (I - T (x) T) vec(P0) = vec(R Q R').
  "unrolled"  cycle reduction itself as ``CR_ITERATIONS`` differentiable iterations (a fixed count, past convergence: the
              iterates A0, A2 underflow to zero and the step becomes the identity), P0 by ``DOUBLING_ITERATIONS`` steps of the
              doubling series X <- X + T_k X T_k', T_k <- T_k^2.

The filter is the loop of oracle/statespace.py (``kalman_filter_logp``) operation for operation: missing-data masks, jitter on F
and P+, the symmetrisations, the ``FilterConventions`` switches.

A full shock covariance enters as (Q + Q') / 2: the gradient is the one of the symmetric parametrisation, entry (i, j) being half
the derivative along E_ij + E_ji for i != j (the oracle itself is not invariant under Q -> Q': R Q R' reaches the filter through
P0 unsymmetrised), which is what ``Q_bar`` "of all k x k entries taken as independent (symmetric)" means (include/dsge_hip.h)."""
import numpy as np
import torch

import oracle
from oracle.statespace import JITTER_DEFAULT, MISSING_FILL

CR_ITERATIONS, DOUBLING_ITERATIONS = 60, 40
CPU = torch.device("cpu")
_LN2PI = float(np.log(2.0 * np.pi))


def _t(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, device=CPU, requires_grad=grad)


def _sym_quad(A, B):
    out = A @ B @ A.T
    return 0.5 * (out + out.T)


def policy_newton(A, B, C):
    """T(A, B, C) around the converged T* of the oracle's cycle reduction: value T* (to the residual's rounding), derivative
    the implicit-function one."""
    Ts, ok, _ = oracle.cycle_reduction_core(A.detach().numpy(), B.detach().numpy(), C.detach().numpy(), 300, 1e-15)
    if not ok:
        raise ArithmeticError("cycle reduction did not converge")
    n = Ts.shape[0]
    Ts = _t(Ts)
    eye = torch.eye(n, dtype=torch.float64, device=CPU)
    M = (B + C @ Ts).detach()
    L = torch.kron(M, eye) + torch.kron(C.detach(), Ts.T.contiguous())  # d vec_r(B X + C X T* + C T* X) / d vec_r(X)
    resid = A + B @ Ts + C @ Ts @ Ts
    return Ts - torch.linalg.solve(L, resid.reshape(-1)).reshape(n, n)


def policy_unrolled(A, B, C, n_iterations=CR_ITERATIONS):
    """cycle_reduction.py's iteration (oracle.cycle_reduction._cr_step) with a fixed trip count."""
    _, ok, n_iter = oracle.cycle_reduction_core(A.detach().numpy(), B.detach().numpy(), C.detach().numpy(), 300, 1e-15)
    if not ok or n_iter + 8 > n_iterations:
        raise ArithmeticError(f"cycle reduction needs {n_iter} iterations: {n_iterations} is not past convergence")
    n = A.shape[0]
    A0, A1, A2, A1_hat = A, B, C, B
    for _ in range(n_iterations):
        X = torch.linalg.solve(A1, torch.cat((A0, A2), dim=1))
        X0, X2 = X[:, :n], X[:, n:]
        m20 = A2 @ X0
        A0, A1, A2, A1_hat = -(A0 @ X0), A1 - A0 @ X2 - m20, -(A2 @ X2), A1_hat - m20
    return -torch.linalg.solve(A1_hat, A)


def lyapunov_kronecker(T, W):
    n = T.shape[0]
    K = torch.eye(n * n, dtype=torch.float64, device=CPU) - torch.kron(T, T)  # vec_r(T X T') = (T (x) T) vec_r(X)
    return torch.linalg.solve(K, W.reshape(-1)).reshape(n, n)


def lyapunov_doubling(T, W, n_iterations=DOUBLING_ITERATIONS):
    X, Tk = W, T
    for _ in range(n_iterations):
        X = X + Tk @ X @ Tk.T
        Tk = Tk @ Tk
    return X


def filter_logp(y, T, R, Q, Z, H, d, P0, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, conventions=None):
    """oracle.kalman_filter_logp's loop on torch tensors (a0 = 0, c = 0); ``y`` is a numpy array."""
    cv = oracle.DEFAULT_CONVENTIONS if conventions is None else conventions
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    m, p = T.shape[0], Z.shape[0]
    a = torch.zeros(m, dtype=torch.float64, device=CPU)
    P = P0
    RQR = R @ Q @ R.T
    RQR_sym = 0.5 * (RQR + RQR.T)
    eye_m = torch.eye(m, dtype=torch.float64, device=CPU)
    eye_p = torch.eye(p, dtype=torch.float64, device=CPU)
    jit_F = jitter if cv.jitter_on_F else 0.0
    jit_P = jitter if cv.jitter_on_P else 0.0
    total = torch.zeros((), dtype=torch.float64, device=CPU)
    for t in range(y.shape[0]):
        yt = y[t]
        miss = np.isnan(yt) | (yt == missing_fill_value)
        keep = _t((~miss).astype(np.float64))
        W = torch.diag(keep)
        Zm = W @ Z
        Hm = W @ H
        ym = _t(np.where(miss, 0.0, yt))

        v = ym - ((d * keep if cv.mask_d else d) + Zm @ a)
        PZt = P @ Zm.T
        F = Zm @ PZt + Hm + jit_F * eye_p
        K = torch.linalg.solve(F.T, PZt.T).T
        IKZ = eye_m - K @ Zm
        a_f = a + K @ v
        if cv.joseph:
            P_f = _sym_quad(IKZ, P) + _sym_quad(K, Hm) + jit_P * eye_m
        else:
            P_f = P - K @ F @ K.T
            P_f = 0.5 * (P_f + P_f.T) + jit_P * eye_m
        if not miss.all():
            inner = v @ torch.linalg.solve(F, v)
            n_const = {"p": p, "observed": int((~miss).sum()), "one": 1}[cv.ll_constant]
            total = total - 0.5 * (n_const * _LN2PI + torch.log(torch.linalg.det(F)) + inner)
        a = T @ a_f
        P = _sym_quad(T, P_f) + RQR_sym
    return total


def logp_and_gradient(A, B, C, D, Z, y, q=None, Q=None, d=None, Hdiag=None, conventions=None, formulation="newton", want_Z=False,
                      jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL):
    """One draw.  ``q`` (k,) diagonal variances or ``Q`` (k, k); ``d``, ``Hdiag`` (p,) or None (= 0, no cotangent returned).
    Returns dict(logp, A_bar, B_bar, C_bar, D_bar, q_bar | Q_bar[, d_bar][, h_bar][, Z_bar]) of numpy arrays."""
    if (q is None) == (Q is None):
        raise ValueError("pass either q or Q")
    p = np.asarray(Z).shape[0]
    leaves = dict(A=_t(A, True), B=_t(B, True), C=_t(C, True), D=_t(D, True), q=_t(q if Q is None else Q, True),
                  d=_t(np.zeros(p) if d is None else d, True), h=_t(np.zeros(p) if Hdiag is None else Hdiag, True), Z=_t(Z, True))
    At, Bt, Ct, Dt = (leaves[x] for x in "ABCD")
    Qt = torch.diag(leaves["q"]) if Q is None else 0.5 * (leaves["q"] + leaves["q"].T)
    T = {"newton": policy_newton, "unrolled": policy_unrolled}[formulation](At, Bt, Ct)
    R = -torch.linalg.solve(Ct @ T + Bt, Dt)
    P0 = {"newton": lyapunov_kronecker, "unrolled": lyapunov_doubling}[formulation](T, R @ Qt @ R.T)
    logp = filter_logp(y, T, R, Qt, leaves["Z"], torch.diag(leaves["h"]), leaves["d"], P0, jitter, missing_fill_value, conventions)
    names = ["A", "B", "C", "D", "q"] + (["d"] if d is not None else []) + (["h"] if Hdiag is not None else []) + (["Z"] if want_Z else [])
    grads = torch.autograd.grad(logp, [leaves[x] for x in names])
    out = {("Q_bar" if x == "q" and Q is not None else x + "_bar"): g.numpy().copy() for x, g in zip(names, grads)}
    out["logp"] = float(logp)
    return out
