"""Device-resident evaluator: torch owns HBM buffers and streams, libdsge_hip does the work.

PyTorch is plumbing here (device memory, the current HIP stream, ``torch.distributed``);
every FLOP of the path runs in the hand-written kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _frontend as F
from . import _lib
from .batched import JITTER_DEFAULT, MISSING_FILL
from .workloads import shard_bounds


def _torch():
    import torch

    return torch


class DeviceBackend:
    """The torch side of ``_frontend``: float64 / int32 CUDA tensors on one device, work enqueued on torch's current stream."""

    host = False

    def __init__(self, torch, device):
        self.torch, self.device = torch, device

    @property
    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def inp(self, t, dtype="float64"):
        if t is not None and not (isinstance(t, self.torch.Tensor) and t.is_cuda and t.dtype == getattr(self.torch, dtype)
                                  and t.is_contiguous()):
            raise ValueError(f"expected a contiguous {dtype} CUDA tensor")
        return t

    def empty(self, shape, dtype="float64"):
        return self.torch.empty(shape, dtype=getattr(self.torch, dtype), device=self.device)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

    def status_io(self, status, nb):
        return self.torch.zeros(nb, dtype=self.torch.int32, device=self.device) if status is None else self.inp(status, "int32")

    # the generated draws of ``_frontend.simulation_smoother``, with torch on the current stream
    @property
    def xp(self):
        return self.torch

    @staticmethod
    def generator(gen):
        return gen  # a torch.Generator of this device, or None for torch's default one

    def randn(self, gen, shape):
        return self.torch.randn(shape, generator=gen, dtype=self.torch.float64, device=self.device)

    def sym_factor(self, A):
        w, V = self.torch.linalg.eigh(self.torch.nan_to_num(A, nan=0.0, posinf=0.0, neginf=0.0))
        return (V * self.torch.sqrt(self.torch.clamp(w, min=0.0))[..., None, :]).contiguous()


class LogpEngine:
    """Fused ``A,B,C,D -> logp`` on one GPU with inputs and outputs resident in HBM.

    All tensor arguments are float64 CUDA tensors on ``device`` (contiguous, row-major,
    leading draw axis); work is enqueued on torch's current stream for that device.
    """

    def __init__(self, device=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.DsgeHipError("LogpEngine needs a GPU: torch.cuda.is_available() is False (no CPU fallback)")
        self.torch = torch
        self.device = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        self.lib = _lib.load()
        self.backend = DeviceBackend(torch, self.device)
        torch.cuda.set_device(self.device)
        _lib.check(self.lib.dsge_set_device(self.device.index or 0))

    # -- helpers ---------------------------------------------------------------------------
    def to_device(self, x, dtype=None):
        torch = self.torch
        if isinstance(x, torch.Tensor):
            return x.to(self.device, dtype or torch.float64).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=self.device)

    def _chk(self, t):
        return self.backend.inp(t)

    _p = staticmethod(DeviceBackend.ptr)

    def _stream(self):
        return self.backend.stream

    def structure_hints(self, A, Z):
        """(n_state_hint, z_selector_hint) from device tensors: one small reduction + host sync;
        the structure is a property of the model, so call this once, not per step."""
        torch = self.torch
        n_state = int(torch.count_nonzero((A != 0).reshape(-1, A.shape[-1]).any(dim=0)).item())
        nz = (Z != 0).reshape(-1, Z.shape[-2], Z.shape[-1])
        sel = bool(((nz.sum(dim=2) == 1).all() & (nz.sum(dim=1) <= 1).all()).item())
        return n_state, int(sel)

    def static_hint(self, A, C):
        """``dsge_options.n_static_hint`` from device tensors: variables whose columns of A and C are exactly zero in
        every draw (one reduction + host sync; a property of the model: call once).  With it the fused call is a pure
        enqueue -- no measuring launch, no read-back inside the library."""
        torch = self.torch
        n = A.shape[-1]
        nz = (A != 0).reshape(-1, n).any(dim=0) | (C != 0).reshape(-1, n).any(dim=0)
        return int(n - torch.count_nonzero(nz).item())

    def record_steady_steps(self, buf):
        """Debug: ``buf`` (int32 CUDA tensor [batch]) receives, from the fast-path Kalman launches that
        follow, the first time step each draw ran in steady-state mode (-1 = never); ``None`` stops."""
        _lib.check(self.lib.dsge_debug_kalman_steady_steps(self._p(self.backend.inp(buf, "int32"))))

    # -- on-device Jacobians ---------------------------------------------------
    def jacobians_from_theta(self, program, theta, out=None):
        """``theta`` (float64 CUDA tensor [batch][npar]) -> (A, B, C, D, q) resident in HBM, evaluated by
        the generated kernel of ``program`` (geconpy_amd.jacobian_codegen.JacobianProgram) on the current
        stream; ``q`` is None when the program carries no shock variances.  ``out`` may hold preallocated
        tensors (A, B, C, D, q) to reuse across MCMC steps."""
        torch = self.torch
        self._chk(theta)
        nb, npar = theta.shape
        if npar != len(program.params):
            raise ValueError(f"theta has {npar} columns, the program has {len(program.params)} parameters")
        n, k = program.n, program.k
        if out is None:
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)  # noqa: E731
            out = (mk(nb, n, n), mk(nb, n, n), mk(nb, n, n), mk(nb, n, k), mk(nb, k) if program.q is not None else None)
        A, B, C, D, q = out
        program.launch(theta.data_ptr(), nb, A.data_ptr(), B.data_ptr(), C.data_ptr(), D.data_ptr(),
                       None if q is None else q.data_ptr(), self._stream())
        return A, B, C, D, q

    def observation_from_theta(self, program, theta, out=None):
        """``theta`` -> (Z [batch][p][n] or None, d [batch][p] or None): the parameter-dependent observation equation of a
        program built with ``Z=`` / ``d=`` (statespace.py:298-388), by its second generated kernel."""
        torch = self.torch
        self._chk(theta)
        nb = theta.shape[0]
        if program.Z is None and program.d is None:
            return None, None
        if out is None:
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)  # noqa: E731
            out = (mk(nb, program.p, program.n) if program.Z is not None else None,
                   mk(nb, program.p) if program.d is not None else None)
        Zb, db = out
        program.launch_obs(theta.data_ptr(), nb, self._p(Zb), self._p(db), self._stream())
        return Zb, db

    def logp_from_theta(self, program, theta, Z, y, d=None, Hdiag=None, jac_out=None, **kw):
        """theta -> A,B,C,D,q -> T,R -> P0 -> logp without the matrices ever leaving the device: the generated
        Jacobian kernel followed by the fused pipeline on the same stream.  Returns (logp, status).  ``Z`` / ``d`` = None
        take the program's own parameter-dependent observation equation (``observation_from_theta``)."""
        A, B, C, D, q = self.jacobians_from_theta(program, theta, out=jac_out)
        if q is None:
            raise ValueError("the program has no shock variances; call jacobians_from_theta + solve_kalman_logp")
        if Z is None or (d is None and getattr(program, "d", None) is not None):
            Zg, dg = self.observation_from_theta(program, theta)
            Z = Zg if Z is None else Z
            d = dg if d is None else d
            if Z is None:
                raise ValueError("no design matrix: pass Z or build the program with Z=")
        return self.solve_kalman_logp(A, B, C, D, q, Z, y, d=d, Hdiag=Hdiag, q_mode=1, **kw)

    def logp_and_grad_from_theta(self, program, theta, Z, y, d=None, Hdiag=None, jac_out=None, grad_out=None,
                                 theta_bar=None, **kw):
        """theta -> (logp, status, d logp / d theta) entirely on the device: generated Jacobian kernel, the fused
        logp + reverse-mode pipeline, and the generated pullback kernel theta_bar = J' (A_bar, B_bar, C_bar, D_bar,
        q_bar) -- the interface a gradient-based sampler (NUTS) needs.  Cotangents of d / Hdiag stay available in the
        returned dict (``grad``)."""
        torch = self.torch
        A, B, C, D, q = self.jacobians_from_theta(program, theta, out=jac_out)
        if q is None:
            raise ValueError("the program has no shock variances")
        # the observation equation: the same resolution as logp_from_theta, so that the pair (logp, gradient) belongs to the
        # SAME function of theta -- a program built with d= filters with its parameter-dependent intercept and the cotangent
        # of d flows back through the generated pullback; a parameter-dependent Z(theta) takes the dense-Z gradient entry
        # point, whose Z_bar goes through the generated pullback of Z
        z_from_program = Z is None and getattr(program, "Z", None) is not None
        d_from_program = d is None and getattr(program, "d", None) is not None
        if z_from_program or d_from_program:
            Zp, dp = self.observation_from_theta(program, theta)
            if z_from_program:
                Z = Zp
            if d_from_program:
                d = dp
        if Z is None:
            raise ValueError("no design matrix: pass Z")
        if z_from_program:
            kw = dict(kw, dense_z=True)
        g = self.solve_kalman_logp_grad(A, B, C, D, q, Z, y, d=d, Hdiag=Hdiag, out=grad_out, **kw)
        if theta_bar is None:
            theta_bar = torch.empty_like(theta)
        program.launch_vjp(theta.data_ptr(), theta.shape[0], g["A_bar"].data_ptr(), g["B_bar"].data_ptr(),
                           g["C_bar"].data_ptr(), g["D_bar"].data_ptr(), g["q_bar"].data_ptr(), theta_bar.data_ptr(),
                           self._stream())
        if d_from_program:  # theta_bar += (d d / d theta)' d_bar
            program.launch_obs_vjp(theta.data_ptr(), theta.shape[0], g["d_bar"].data_ptr(), theta_bar.data_ptr(), self._stream())
        if z_from_program:  # theta_bar += (d Z / d theta)' Z_bar
            program.launch_obs_z_vjp(theta.data_ptr(), theta.shape[0], g["Z_bar"].data_ptr(), theta_bar.data_ptr(), self._stream())
        return g["logp"], g["status"], theta_bar, g

    # -- product entry points --------------------------------------------------------------
    def solve_kalman_logp(self, A, B, C, D, Q, Z, y, d=None, Hdiag=None, q_mode=None, solver="cycle_reduction",
                          tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL,
                          logp=None, status=None, n_state_hint=0, z_selector_hint=0, n_lead_hint=0, T_out=None,
                          R_out=None, options=None):
        """Enqueue one fused evaluation of the whole batch; returns (logp, status) tensors
        (asynchronous: synchronize the stream before reading them on the host).  ``T_out`` [batch][n][n] /
        ``R_out`` [batch][n][k]: optional float64 CUDA tensors that receive the policy matrices."""
        hints = dict(n_state_hint=n_state_hint, z_selector_hint=z_selector_hint, n_lead_hint=n_lead_hint)
        out = F.solve_kalman_logp(self.backend, A, B, C, D, Q, Z, y, d=d, Hdiag=Hdiag, q_mode=q_mode, solver=solver, tol=tol,
                                  max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value, hints=lambda a: hints,
                                  options=options, out=dict(logp=logp, status=status, T=T_out, R=R_out))
        return out["logp"], out["status"]

    def kalman_smoother(self, T, R, Q, Z, y, d=None, Hdiag=None, q_mode=None, jitter=JITTER_DEFAULT,
                        missing_fill_value=MISSING_FILL, full_covariances=False, covariances=True, rank_tol=None,
                        scratch_limit_bytes=None, status=None, options=None):
        """Smoothed states, covariances and shocks of the whole batch (``dsge_kalman_smoother_batched``; see
        ``batched.kalman_smoother_batched``) from device tensors T [batch][m][m], R [batch][m][k], on torch's current stream.
        Returns a dict of device tensors: ll, smoothed_states, smoothed_covs (None with ``covariances=False``: the covariance
        recursion is then skipped), smoothed_shocks, status (asynchronous: synchronize before reading on the host).  ``status``:
        optional int32 tensor [batch] of incoming per-draw status words (updated in place)."""
        return F.kalman_smoother(self.backend, "kalman_smoother", T, R, Q, Z, y, d=d, Hdiag=Hdiag, q_mode=q_mode, status=status,
                                 jitter=jitter, missing_fill=missing_fill_value, cov=covariances, full=full_covariances,
                                 rank_tol=rank_tol, scratch_limit_bytes=scratch_limit_bytes, options=options)

    def kalman_logp_segments(self, T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                             jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, options=None, outputs=F.SEGMENT_OUTPUTS,
                             q_mode=None, status=None, out=None):
        """Kalman log-likelihood across dated structural breaks of the whole batch (``dsge_kalman_logp_segments_batched``; see
        ``batched.kalman_logp_segments_batched``) from device tensors, on torch's current stream.  ``seg_start`` is a HOST list
        (passed to the kernel by value: the call is a pure enqueue).  ``out``: optional dict with preallocated ``logp`` / ``ll`` /
        ``a_last`` / ``P_last``.  Returns dict(logp, ll, a_last, P_last, status) of device tensors; asynchronous."""
        return F.kalman_logp_segments(self.backend, "kalman_logp_segments", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d, a0=a0, P0=P0,
                                      shift=shift, q_mode=q_mode, status=status, jitter=jitter, missing_fill=missing_fill_value,
                                      options=options, outputs=outputs, out=out)

    def solve_kalman_logp_segments(self, A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                   solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                   missing_fill_value=MISSING_FILL, options=None, outputs=F.SEGMENT_OUTPUTS, q_mode=None,
                                   n_lead_hint=0, out=None):
        """``A .. D`` [batch][S][n][n|k] -> T, R per (draw, segment) by the existing solver entries on the flattened batch, the
        segments' status words ORed per draw with tensor operations, then ``kalman_logp_segments``
        (``batched.solve_kalman_logp_segments_batched``).  Returns its dict plus ``T`` and ``R``; asynchronous."""
        return F.solve_kalman_logp_segments(self.backend, "solve_kalman_logp_segments", A, B, C, D, q, Z, y, seg_start, solver=solver,
                                            tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options, Hdiag=Hdiag, d=d,
                                            a0=a0, P0=P0, shift=shift, q_mode=q_mode, jitter=jitter, missing_fill=missing_fill_value,
                                            outputs=outputs, out=out)

    def kalman_logp_segments_grad(self, T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                  jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, scratch_limit_bytes=None, options=None,
                                  outputs=F.SEGMENT_GRADIENT_OUTPUTS, q_mode=None, status=None, out=None):
        """``logp`` across dated structural breaks and its gradient with respect to every input
        (``dsge_kalman_logp_segments_grad_batched``; see ``batched.kalman_logp_segments_grad_batched``) from device tensors, on
        torch's current stream.  ``seg_start`` is a HOST list.  ``out``: optional dict of preallocated outputs (``logp`` and the
        names of ``outputs``).  Returns a dict of device tensors (None where not asked for) and status; asynchronous."""
        return F.kalman_logp_segments_grad(self.backend, "kalman_logp_segments_grad", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d,
                                           a0=a0, P0=P0, shift=shift, q_mode=q_mode, status=status, jitter=jitter,
                                           missing_fill=missing_fill_value, scratch_limit_bytes=scratch_limit_bytes,
                                           options=options, outputs=outputs, out=out)

    def solve_kalman_logp_segments_grad(self, A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                        solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                        missing_fill_value=MISSING_FILL, scratch_limit_bytes=None, options=None,
                                        outputs=F.SEGMENT_GRADIENT_OUTPUTS, q_mode=None, n_lead_hint=0, out=None):
        """``A .. D`` [batch][S][n][n|k] (n <= 56) solved as ``solve_kalman_logp_segments`` solves them, ``kalman_logp_segments_grad``,
        then the adjoint entries on the flattened batch (``batched.solve_kalman_logp_segments_grad_batched``): its dict plus
        ``A_bar`` .. ``D_bar``, ``T`` and ``R``.  Failed draws are ORed and zeroed with tensor operations; asynchronous."""
        return F.solve_kalman_logp_segments_grad(self.backend, "solve_kalman_logp_segments_grad", A, B, C, D, q, Z, y, seg_start,
                                                 solver=solver, tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options,
                                                 Hdiag=Hdiag, d=d, a0=a0, P0=P0, shift=shift, q_mode=q_mode, jitter=jitter,
                                                 missing_fill=missing_fill_value, scratch_limit_bytes=scratch_limit_bytes,
                                                 outputs=outputs, out=out)

    def kalman_smoother_segments(self, T, R, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                 jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, full_covariances=False, rank_tol=None,
                                 scratch_limit_bytes=None, options=None, outputs=F.SEGMENT_SMOOTHER_OUTPUTS, q_mode=None, status=None,
                                 out=None):
        """Smoothed states, covariances and shocks across dated structural breaks, with the per-step filter outputs
        (``dsge_kalman_smoother_segments_batched``; see ``batched.kalman_smoother_segments_batched``) from device tensors, on torch's
        current stream.  ``seg_start`` is a HOST list.  ``out``: optional dict of preallocated outputs, by the names of ``outputs``.
        ``status``: optional int32 tensor [batch] of incoming status words (updated in place).  Returns a dict of device tensors
        (None where not asked for) and status; asynchronous."""
        return F.kalman_smoother_segments(self.backend, "kalman_smoother_segments", T, R, q, Z, y, seg_start, Hdiag=Hdiag, d=d, a0=a0,
                                          P0=P0, shift=shift, q_mode=q_mode, status=status, jitter=jitter,
                                          missing_fill=missing_fill_value, full=full_covariances, rank_tol=rank_tol,
                                          scratch_limit_bytes=scratch_limit_bytes, options=options, outputs=outputs, out=out)

    def solve_kalman_smoother_segments(self, A, B, C, D, q, Z, y, seg_start, Hdiag=None, d=None, a0=None, P0=None, shift=None,
                                       solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT,
                                       missing_fill_value=MISSING_FILL, full_covariances=False, rank_tol=None,
                                       scratch_limit_bytes=None, options=None, outputs=F.SEGMENT_SMOOTHER_OUTPUTS, q_mode=None,
                                       n_lead_hint=0, out=None):
        """``A .. D`` [batch][S][n][n|k] solved as ``solve_kalman_logp_segments`` solves them, then ``kalman_smoother_segments``
        (``batched.solve_kalman_smoother_segments_batched``).  Returns its dict plus ``T`` and ``R``; asynchronous."""
        return F.solve_kalman_smoother_segments(self.backend, "solve_kalman_smoother_segments", A, B, C, D, q, Z, y, seg_start,
                                                solver=solver, tol=tol, max_iter=max_iter, n_lead_hint=n_lead_hint, options=options,
                                                Hdiag=Hdiag, d=d, a0=a0, P0=P0, shift=shift, q_mode=q_mode, jitter=jitter,
                                                missing_fill=missing_fill_value, full=full_covariances, rank_tol=rank_tol,
                                                scratch_limit_bytes=scratch_limit_bytes, outputs=outputs, out=out)

    def stationary_factor(self, T, R, Q, q_mode=None):
        """F [batch][m][m] with F F' = P0 per draw (``batched.stationary_factor``) from device tensors: ``dsge_lyapunov_batched``
        and a batched ``torch.linalg.eigh``, on torch's current stream."""
        return F.stationary_factor(self.backend, "stationary_factor", T, R, Q, q_mode=q_mode)

    def simulation_smoother(self, T, R, Q, Z, y, n_paths=1, d=None, Hdiag=None, q_mode=None, x0=None, eps=None, eta=None,
                            generator=None, return_draws=False, status=None, jitter=JITTER_DEFAULT,
                            missing_fill_value=MISSING_FILL, rank_tol=None, scratch_limit_bytes=None, options=None):
        """Joint posterior draws of the state paths and shocks of the whole batch (``dsge_simulation_smoother_batched``; see
        ``batched.simulation_smoother_batched``) from device tensors, on torch's current stream.  Draw arrays that are None are
        made on the device from ``generator`` (a ``torch.Generator`` of this device; None: torch's default).  Returns a dict of
        device tensors: states, shocks, ll, status[, x0, eps, eta]; asynchronous."""
        return F.simulation_smoother(self.backend, "simulation_smoother", T, R, Q, Z, y, n_paths=n_paths, d=d, Hdiag=Hdiag,
                                     q_mode=q_mode, x0=x0, eps=eps, eta=eta, rng=generator, return_draws=return_draws, status=status,
                                     jitter=jitter, missing_fill=missing_fill_value, rank_tol=rank_tol,
                                     scratch_limit_bytes=scratch_limit_bytes, options=options)

    # -- post-solve dynamics (csrc/dsge_dynamics.hpp) -----------------------------------------
    def simulate(self, T, R, eps, n_steps=None, x0=None, status=None, out=None):
        """Simulated paths of the whole batch from device tensors (``dsge_simulate_batched``; see
        ``batched.simulate_batched``), enqueued on torch's current stream.  ``eps``: (n_paths, n_shock_steps, k) or
        (batch, n_paths, n_shock_steps, k) -- draw it with torch on the device.  Returns the paths
        (batch, n_paths, n_steps, m) (``out`` if given); asynchronous."""
        return F.simulate(self.backend, "simulate", T, R, eps, n_steps=n_steps, x0=x0, status=status, out=out)

    def impulse_response(self, T, R, n_steps=40, S=None, weights=None, fevd=False, irf=True, status=None, out=None):
        """Impulse responses (and, with ``fevd=True``, their variance decomposition) of the whole batch from device tensors
        (``dsge_irf_batched``; see ``batched.impulse_response_batched``), on torch's current stream.  ``out``: optional dict
        with preallocated ``irf`` / ``fevd`` tensors.  Returns dict(irf (batch, c, n_steps, m) or None,
        fevd (batch, n_steps, m, c) or None); asynchronous."""
        return F.impulse_response(self.backend, "impulse_response", T, R, n_steps=n_steps, S=S, weights=weights, fevd=fevd, irf=irf,
                                  status=status, out=out)

    def forecast(self, T, R, Q, a0, P0=None, n_steps=10, Z=None, d=None, Hdiag=None, q_mode=None, covariances="diag",
                 status=None, out=None):
        """Forecast moments of the whole batch from device tensors (``dsge_forecast_batched``; see
        ``batched.forecast_batched``), on torch's current stream.  ``out``: optional dict with preallocated ``states`` / ``covs``
        / ``observed`` / ``observed_covs``.  Returns that dict (entries not requested are None); asynchronous."""
        return F.forecast(self.backend, "forecast", T, R, Q, a0, P0=P0, n_steps=n_steps, Z=Z, d=d, Hdiag=Hdiag, q_mode=q_mode,
                          covariances=covariances, status=status, out=out)

    # -- historical shock decomposition (csrc/dsge_shock_decomp.hpp) ------------------------------
    def shock_decomposition(self, T, R, states, shocks, groups=None, variables=None, Z=None, remainder=True, status=None, out=None):
        """Historical shock decomposition of the whole batch from device tensors (``dsge_shock_decomposition_batched``; see
        ``batched.shock_decomposition_batched``), one launch on torch's current stream.  From ``kalman_smoother``: ``states =
        s["smoothed_states"], shocks = s["smoothed_shocks"]``; from ``simulation_smoother``: ``s["states"], s["shocks"]``.
        ``groups`` / ``variables`` are host index lists.  ``out``: optional dict with preallocated ``contributions`` /
        ``observed``.  Returns dict(contributions, observed or None, components); asynchronous."""
        return F.shock_decomposition(self.backend, "shock_decomposition", T, R, states, shocks, groups=groups, variables=variables,
                                     Z=Z, remainder=remainder, status=status, out=out)

    # -- conditional forecast (csrc/dsge_condfc.hpp) ---------------------------------------------
    def conditional_forecast(self, T, R, Q, x0, conditions, n_steps, Z=None, d=None, eps=None, n_paths=None, free_shocks=None,
                             q_mode=None, status=None, rank_tol=0.0, out=None):
        """Conditional forecasts of the whole batch from device tensors (``dsge_conditional_forecast_batched``; see
        ``batched.conditional_forecast_batched``), on torch's current stream.  ``conditions`` as a tensor with NaN = free is read
        back once to find the pattern (a synchronisation); the triple ``(cond_t, cond_j, values)`` with host index lists and a
        device tensor of values is asynchronous.  ``status`` (device int32) is updated in place.  ``out``: optional dict with
        preallocated ``x`` / ``shocks`` / ``observed``.  Returns dict(x, shocks, observed, status)."""
        return F.conditional_forecast(self.backend, "conditional_forecast", T, R, Q, x0, conditions, n_steps, Z=Z, d=d, eps=eps,
                                      n_paths=n_paths, free_shocks=free_shocks, q_mode=q_mode, status=status, rank_tol=rank_tol,
                                      out=out)

    # -- spectral densities and filtered moments (csrc/dsge_spectral.hpp) --------------------------
    def spectral_moments(self, T, R, Q, n_grid=512, n_lags=10, Z=None, Hdiag=None, gain=None, correlation=False, spectrum=False,
                         q_mode=None, status=None, rank_tol=None, scratch_limit_bytes=None, acov=True, out=None):
        """Spectral densities and filtered autocovariances of the whole batch from device tensors
        (``dsge_spectral_moments_batched``; see ``batched.spectral_moments_batched``), on torch's current stream.  ``gain`` is a
        device tensor (``torch.as_tensor(batched.hp_gain(n_grid), device=...)``).  ``status`` (device int32) is updated in place.
        ``out``: optional dict with preallocated ``acov`` / ``spectrum`` (complex128).  ``freqs`` comes back as a host array."""
        return F.spectral_moments(self.backend, "spectral_moments", T, R, Q, n_grid=n_grid, n_lags=n_lags, Z=Z, Hdiag=Hdiag,
                                  gain=gain, correlation=correlation, spectrum=spectrum, acov=acov, q_mode=q_mode, status=status,
                                  rank_tol=rank_tol, scratch_limit_bytes=scratch_limit_bytes, out=out)

    # -- anticipated shocks (csrc/dsge_anticipated.hpp) -------------------------------------------
    def anticipated_paths(self, B, C, T, R, eps, n_steps=None, mode="perfect_foresight", x0=None, Z=None, d=None, status=None,
                          rank_tol=0.0, outputs=("x",), out=None):
        """Paths with anticipated shocks (perfect foresight or news) of the whole batch from device tensors
        (``dsge_anticipated_paths_batched``; see ``batched.anticipated_paths_batched``), on torch's current stream.  ``status``
        (device int32) is updated in place.  ``out``: optional dict with preallocated ``x`` / ``w`` / ``observed`` / ``G``.
        Returns dict(those of x, w, observed, G that ``outputs`` names, status); asynchronous."""
        return F.anticipated_paths(self.backend, "anticipated_paths", B, C, T, R, eps, n_steps=n_steps, mode=mode, x0=x0, Z=Z, d=d,
                                   status=status, rank_tol=rank_tol, outputs=outputs, out=out)

    # -- occasionally binding bound (csrc/dsge_obc.hpp) -------------------------------------------
    def constrained_paths(self, B, C, T, R, eps, c, bound, shock, horizon, n_steps=None, x0=None, Z=None, d=None, status=None,
                          rank_tol=0.0, max_iter=0, outputs=("x",), out=None):
        """Perfect-foresight paths under an occasionally binding bound of the whole batch from device tensors
        (``dsge_constrained_paths_batched``; see ``batched.constrained_paths_batched``), on torch's current stream.  ``bound``: a
        number or a device tensor (batch,).  ``status`` (device int32) is updated in place.  ``out``: optional dict with preallocated
        outputs.  Returns dict(those of x, w, observed, nu, gap, Mz, path_status, iters that ``outputs`` names, status); asynchronous."""
        return F.constrained_paths(self.backend, "constrained_paths", B, C, T, R, eps, c, bound, shock, horizon, n_steps=n_steps, x0=x0,
                                   Z=Z, d=d, status=status, rank_tol=rank_tol, max_iter=max_iter, outputs=outputs, out=out)

    # -- stochastic simulation at the bound (csrc/dsge_obc_sim.hpp) --------------------------------
    def constrained_simulate(self, B, C, T, R, eps, c, bound, shock, horizon, n_steps=None, x0=None, Z=None, d=None, status=None,
                             rank_tol=0.0, max_iter=0, outputs=("x",), out=None):
        """Stochastic simulation at an occasionally binding bound of the whole batch from device tensors
        (``dsge_constrained_simulate_batched``; see ``batched.constrained_simulate_batched``), on torch's current stream: surprise
        shocks, the plan re-solved every period inside one kernel.  ``bound``: a number or a device tensor (batch,).  ``status``
        (device int32) is updated in place.  ``out``: optional dict with preallocated outputs.  Returns dict(those of x, observed, gap,
        shadow, plan, duration, iters, Mz, path_status, fail_step that ``outputs`` names, status); asynchronous."""
        return F.constrained_simulate(self.backend, "constrained_simulate", B, C, T, R, eps, c, bound, shock, horizon, n_steps=n_steps,
                                      x0=x0, Z=Z, d=d, status=status, rank_tol=rank_tol, max_iter=max_iter, outputs=outputs, out=out)

    # -- second-order dynamics (csrc/dsge_pruned.hpp) -------------------------------------------
    def simulate_pruned(self, *args, out=None, **kwargs):
        """Simulated paths of the pruned second-order system from device tensors (``dsge_simulate_pruned_batched``; arguments as
        ``batched.simulate_pruned_batched``: the seven solution arguments or one dict of them, then ``eps, n_steps=None, x0=None,
        status=None, parts=False``), on torch's current stream.  ``S`` is a host index list (``second_order_structure``).  ``out``:
        optional dict with preallocated ``x`` / ``x_f`` / ``x_s``.  Returns dict(x[, x_f, x_s]); asynchronous."""
        sol, r = F.bind_solution("simulate_pruned", args, kwargs,
                                 (("eps", None), ("n_steps", None), ("x0", None), ("status", None), ("parts", False)))
        return F.simulate_pruned(self.backend, sol, r["eps"], n_steps=r["n_steps"], x0=r["x0"], status=r["status"], parts=r["parts"],
                                 out=out)

    def girf_pruned(self, *args, out=None, **kwargs):
        """Generalised impulse responses of the pruned second-order system from device tensors (``dsge_girf_pruned_batched``;
        arguments as ``batched.girf_pruned_batched``), on torch's current stream.  ``out``: an optional preallocated tensor.
        Returns dict(girf (batch, c, n_steps, n)); asynchronous."""
        sol, r = F.bind_solution("girf_pruned", args, kwargs,
                                 (("n_steps", 40), ("impulses", None), ("eps", None), ("x0", None), ("status", None)))
        return dict(girf=F.girf_pruned(self.backend, sol, n_steps=r["n_steps"], impulses=r["impulses"], eps=r["eps"], x0=r["x0"],
                                       status=r["status"], out=out))

    def solve_kalman_logp_grad(self, A, B, C, D, q, Z, y, d=None, Hdiag=None, solver="cycle_reduction", tol=1e-6, max_iter=50,
                               jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, n_filter_hint=0, n_lead_hint=0,
                               out=None, options=None, full_covariance=False, dense_z=False):
        """logp and its reverse-mode gradient for the whole batch, device-resident (dsge_solve_kalman_logp_grad_batched).
        ``q``: (k,) or (batch, k) diagonal shock variances; with ``full_covariance=True`` a full symmetric Q, (k, k) or
        (batch, k, k) (statespace.py:247-251), and ``q_bar`` is (batch, k, k).  Returns a dict of tensors: logp, status, A_bar,
        B_bar, C_bar, D_bar, q_bar[, d_bar][, h_bar] (asynchronous).  ``out`` may carry the same dict from an earlier call to
        reuse the buffers.  ``dense_z=True``: any design matrix (observation equations), through
        ``dsge_solve_kalman_logp_grad_dense_z_batched`` (n + p <= 56); the dict then also holds ``Z_bar`` (batch, p, n) and
        ``n_filter_hint`` counts the state variables (non-zero columns of A)."""
        route = dict(dense_z=dense_z, Z_bar=dense_z, n_hint=n_filter_hint, n_lead_hint=n_lead_hint)
        return F.solve_kalman_logp_grad(self.backend, A, B, C, D, q, Z, y, full=full_covariance, d=d, Hdiag=Hdiag, solver=solver, tol=tol,
                                        max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value, route=lambda a: route,
                                        options=options, out=out)

    def second_order_structure(self, A, C, Z):
        """(S, L, U) int32 numpy index lists of ``batched.second_order_structure`` from device tensors (a property of the
        model: one reduction + host sync, call once)."""
        n = A.shape[-1]
        nzA = (A != 0).reshape(-1, n).any(dim=0).cpu().numpy()
        nzC = (C != 0).reshape(-1, n).any(dim=0).cpu().numpy()
        nzZ = (Z != 0).reshape(-1, n).any(dim=0).cpu().numpy()
        S = np.flatnonzero(nzA)
        U = np.concatenate([S, np.setdiff1d(np.flatnonzero(nzZ), S)])
        return S.astype(np.int32), np.flatnonzero(nzC).astype(np.int32), U.astype(np.int32)

    def second_order_logp(self, A, B, C, D, hess_idx, hess_val, q, Z, y, structure, d=None, Hdiag=None,
                          solver="cycle_reduction", tol=1e-8, max_iter=1000, jitter=JITTER_DEFAULT,
                          missing_fill_value=MISSING_FILL, logp=None, status=None, stage_ms=None, options=None):
        """Second-order perturbation + pruned-state-space quasi-likelihood of the whole batch, device-resident
        (include/dsge_hip.h: ``dsge_second_order_logp_batched``; BASELINE configs[4]).  ``hess_idx``: int32 CUDA tensor
        (nnz, 3); ``hess_val``: float64 (batch, nnz); ``q``: (k,) or (batch, k); ``structure`` = ``second_order_structure``.
        ``stage_ms``: a ctypes float[4] that receives the stage durations (synchronises).  Returns (logp, status)."""
        out, _ = F.second_order_logp(self.backend, A, B, C, D, hess_idx, hess_val, q, Z, y, d=d, Hdiag=Hdiag, solver=solver, tol=tol,
                                     max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value, structure=structure,
                                     options=options, out=dict(logp=logp, status=status),
                                     stage_ms=None if stage_ms is None else ctypes.addressof(stage_ms))
        return out["logp"], out["status"]

    def profile_kernels(self, A, B, C, D, Q, Z, y, d=None, Hdiag=None, q_mode=None, solver="cycle_reduction",
                        tol=1e-6, max_iter=50, jitter=JITTER_DEFAULT, missing_fill_value=MISSING_FILL, reps=5,
                        n_state_hint=0, z_selector_hint=0, n_lead_hint=0):
        """Average per-kernel durations (ms) measured with HIP events on the launch stream:
        dict(solver=, assemble=, kalman=)."""
        b = self.backend
        a = F.model_args(b, A, B, C, D, y)
        nb, n, k = a["batch"], a["n"], a["k"]
        a.update(F.obs_args(b, Z, d, Hdiag, nb, a["p"], n))
        logp, status = b.empty((nb,)), b.empty((nb,), "int32")
        ms = (ctypes.c_float * 3)()
        F.call(b, "dsge_profile_pipeline", **a, Q=b.inp(Q), q_mode=F.q_layout(Q.shape, q_mode, nb, k), solver=_lib.SOLVER_CODES[solver],
               tol=tol, max_iter=max_iter, jitter=jitter, missing_fill=missing_fill_value, n_state_hint=n_state_hint,
               z_selector_hint=z_selector_hint, n_lead_hint=n_lead_hint, logp_out=logp, status_out=status, reps=reps,
               ms_out=ctypes.addressof(ms))
        return dict(solver=float(ms[0]), assemble=float(ms[1]), kalman=float(ms[2]))


class ShardedLogpEvaluator:
    """Draw-sharded evaluation across the ranks of a ``torch.distributed`` group.

    Rank r owns the contiguous draws ``[lo_r, hi_r)`` (``workloads.shard_bounds``), evaluates
    them locally with ``local_eval`` and the per-draw (logp, status) are all-gathered into
    rank-ordered buffers, so ``logp[i]`` is bit-exactly draw i on every rank (stricter than
    the reference's ``imap_unordered`` pool, perturbation_diagnostics.py:484-489).  There is
    no data-path collective besides that gather.

    ``local_eval(lo, hi) -> (logp, status)`` returns 1-D tensors of length hi-lo on
    ``device``; the product path passes a closure over ``LogpEngine.solve_kalman_logp``.
    """

    def __init__(self, global_batch, local_eval, device, group=None):
        import torch.distributed as dist

        torch = _torch()
        self.torch = torch
        self.dist = dist
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.global_batch = int(global_batch)
        self.local_eval = local_eval
        self.device = device
        self.bounds = [shard_bounds(self.global_batch, self.world, r) for r in range(self.world)]
        self.lo, self.hi = self.bounds[self.rank]
        self.max_shard = max(hi - lo for lo, hi in self.bounds)
        # ONE collective per step: each rank contributes one byte record [logp f64 x m | status i32 x m | pad]
        m = self.max_shard
        self._rec = 8 * m + 4 * m + (-(12 * m) % 8)
        # RCCL gathers device buffers in place over xGMI; a gloo group (CPU tests, several ranks sharing one device)
        # stages the 12-byte-per-draw records through the host
        self.host_staged = bool(self.distributed and dist.get_backend(group) != "nccl" and
                                torch.device(device).type != "cpu")
        buf_dev = "cpu" if self.host_staged else device
        self._l_buf = torch.zeros(self._rec, dtype=torch.uint8, device=buf_dev)
        self._g_buf = torch.empty(self.world * self._rec, dtype=torch.uint8, device=buf_dev)
        self._l_logp = self._l_buf[: 8 * m].view(torch.float64)
        self._l_stat = self._l_buf[8 * m : 12 * m].view(torch.int32)
        self._l_logp.fill_(float("nan"))
        n_loc = self.hi - self.lo
        # the rank's slice of the send record: a ``local_eval`` that writes its logp / status straight into these (device views when
        # the group is RCCL) saves the two staging copies of every step
        self.local_logp = self._l_logp[:n_loc]
        self.local_status = self._l_stat[:n_loc]
        self._even = all(hi - lo == m for lo, hi in self.bounds)
        self._on_device = not self.host_staged

    def step(self):
        """Evaluate the local shard and gather; returns (logp, status) for ALL draws.  Per step: the local evaluation, ONE
        ``all_gather_into_tensor`` of the packed records, and one unpacking copy per output (the gathered records interleave logp
        and status per rank); no staging copy when ``local_eval`` wrote into ``local_logp`` / ``local_status``, no device transfer
        when the group gathers on the device."""
        logp, status = self.local_eval(self.lo, self.hi)
        if self.world == 1:
            return logp, status
        if logp.data_ptr() != self.local_logp.data_ptr():
            self.local_logp.copy_(logp)
        if status.data_ptr() != self.local_status.data_ptr():
            self.local_status.copy_(status)
        self.dist.all_gather_into_tensor(self._g_buf, self._l_buf, group=self.group)
        torch = self.torch
        m = self.max_shard
        recs = self._g_buf.view(self.world, self._rec)
        g_logp = recs[:, : 8 * m].view(torch.float64)        # (world, m) strided views of the gathered records
        g_stat = recs[:, 8 * m : 12 * m].view(torch.int32)
        if self._even:
            out_l, out_s = g_logp.reshape(-1), g_stat.reshape(-1)
        else:
            out_l = torch.cat([g_logp[r, : hi - lo] for r, (lo, hi) in enumerate(self.bounds)])
            out_s = torch.cat([g_stat[r, : hi - lo] for r, (lo, hi) in enumerate(self.bounds)])
        if self._on_device:
            return out_l, out_s
        return out_l.to(self.device), out_s.to(self.device)
