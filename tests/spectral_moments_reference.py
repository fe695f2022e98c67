"""The definition of ``dsge_spectral_moments_batched`` in plain numpy (TEST INFRASTRUCTURE ONLY; a helper, not a test module):
complex128 ``np.linalg.solve`` per draw and frequency, nothing shared with the device code."""
import numpy as np


def q_matrix(Q, q_mode, b, k):
    """The (k, k) shock covariance of draw ``b`` from one of the four layouts "diag" / "diag_batched" / "full" / "full_batched"."""
    Q = np.asarray(Q, dtype=np.float64)
    q = Q[b] if q_mode.endswith("_batched") else Q
    return np.diag(q) if q_mode.startswith("diag") else q


def solved_frequencies(n_grid, gain, spectrum):
    """The indices n the entry solves: all with the spectrum wanted or no gain, else those of non-zero gain."""
    nf = n_grid // 2 + 1
    return np.arange(nf) if gain is None or spectrum else np.flatnonzero(np.asarray(gain) != 0.0)


def spectral_moments(T, R, Q, q_mode, n_grid, n_lags, Z=None, Hdiag=None, gain=None, correlation=False, spectrum=True):
    """dict(acov (nb, n_lags + 1, dim, dim), spectrum (nb, nf, dim, dim) complex with NaN where a frequency is not solved,
    cond (nb,): the largest 2-norm condition number of I - exp(-i w_n) T over the solved frequencies)."""
    nb, m, k = R.shape
    N, nf = n_grid, n_grid // 2 + 1
    w = 2.0 * np.pi * np.arange(nf) / N
    g = np.ones(nf) if gain is None else np.asarray(gain, dtype=np.float64)
    cn = np.where((np.arange(nf) == 0) | (2 * np.arange(nf) == N), 1.0, 2.0)
    todo = solved_frequencies(N, gain, spectrum)
    dim = m if Z is None else Z.shape[-2]
    acov = np.zeros((nb, n_lags + 1, dim, dim))
    spec = np.full((nb, nf, dim, dim), np.nan + 1j * np.nan)
    cond = np.zeros(nb)
    for b in range(nb):
        Zm = np.eye(m) if Z is None else (Z[b] if Z.ndim == 3 else Z)
        Hd = None if Hdiag is None else (Hdiag[b] if Hdiag.ndim == 2 else Hdiag)
        Qb = q_matrix(Q, q_mode, b, k)
        for n in todo:
            A = np.eye(m) - np.exp(-1j * w[n]) * T[b]
            cond[b] = max(cond[b], np.linalg.cond(A))
            H = Zm @ np.linalg.solve(A, R[b].astype(np.complex128))
            F = H @ Qb @ H.conj().T
            if Hd is not None:
                F = F + np.diag(Hd)
            spec[b, n] = F / (2.0 * np.pi)
            if g[n] != 0.0:
                for j in range(n_lags + 1):
                    acov[b, j] += cn[n] * g[n] * np.real(F * np.exp(1j * w[n] * j)) / N
        if correlation:
            sd = np.sqrt(np.diag(acov[b, 0]))
            acov[b] = acov[b] / np.outer(sd, sd)
    return dict(acov=acov, spectrum=spec, cond=cond)
