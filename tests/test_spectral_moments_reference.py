"""CPU: the numpy reference of the spectral moments (tests/spectral_moments_reference.py) against independent formulations -- the
Lyapunov route for a unit gain, a time-domain identity without complex arithmetic for any gain, real solves at the two real
frequencies, and a finer grid for the HP filter.  Bar: 1e-10 of max|acov[0]| (of max|spectrum| for the spectrum)."""
import functools

import numpy as np
import pytest
import scipy.linalg

from geconpy_amd import batched
from tests import spectral_moments_cases as cases
from tests import spectral_moments_reference as ref

BAR = 1e-10
ACCURACY_CASES = tuple(n for n in cases.NAMES)


def _draw_inputs(kw, b):
    T, R = kw["T"][b], kw["R"][b]
    m, k = R.shape
    Q = ref.q_matrix(kw["Q"], kw["q_mode"], b, k)
    Z = kw["Z"]
    Zm = np.eye(m) if Z is None else (Z[b] if Z.ndim == 3 else Z)
    H = kw["Hdiag"]
    Hd = np.zeros(Zm.shape[0]) if H is None else (H[b] if H.ndim == 2 else H)
    return T, R, Q, Zm, Hd


def _reference(kw, **over):
    kw = {**kw, **over}
    kw.pop("acov")
    return ref.spectral_moments(kw.pop("T"), kw.pop("R"), kw.pop("Q"), kw.pop("q_mode"), kw.pop("n_grid"), kw.pop("n_lags"), **kw)


@pytest.mark.parametrize("name", ACCURACY_CASES)
def test_the_pencils_of_the_cases_are_well_conditioned(name):
    assert cases.reference(name)["cond"].max() <= cases.COND_BOUND


def _folded_autocovariances(T, R, Q, Zm, Hd, N):
    """Gamma°_j = sum_q Gamma_{j + q N}, j = 0 .. N-1, of w = Zm x + noise: P, powers of T and (I - T^N)^-1, all real."""
    m = T.shape[0]
    P = scipy.linalg.solve_discrete_lyapunov(T, R @ Q @ R.T)
    S = np.linalg.solve(np.eye(m) - np.linalg.matrix_power(T, N), P)  # (I - T^N)^-1 P
    pw = [np.eye(m)]
    for _ in range(N):
        pw.append(pw[-1] @ T)
    G = np.stack([Zm @ (pw[j] @ S + (pw[N - j] @ S).T) @ Zm.T for j in range(N)])
    G[0] += np.diag(Hd)
    return G


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n != "sw17_unit_root"])
def test_unit_gain_is_the_lyapunov_route(name):
    """N = 256 (1024 for full_nk).  Every draw against the autocovariances FOLDED modulo N, which is the definition; a draw whose
    aliasing rho(T)^N is below 1e-13 (draw 0 of every model is) also against the plain ``Zm T^j P Zm' (+H)``.  Draws 1 and 2 of
    sw16 / sw17 have rho = 0.921 / 0.922, rho^256 = 7e-10 / 1e-9: there the plain form differs by 1e-9, as it must."""
    kw = cases.case(name)
    N = 1024 if name == "nk_persistent" else 256
    r = _reference(kw, n_grid=N, n_lags=1, gain=None, correlation=False, spectrum=False)
    plain = 0
    for b in range(cases.NB):
        T, R, Q, Zm, Hd = _draw_inputs(kw, b)
        want = _folded_autocovariances(T, R, Q, Zm, Hd, N)[:2]
        assert np.abs(r["acov"][b] - want).max() <= BAR * np.abs(want[0]).max()
        if np.abs(np.linalg.eigvals(T)).max() ** N <= 1e-13:
            P = scipy.linalg.solve_discrete_lyapunov(T, R @ Q @ R.T)
            want = np.stack([Zm @ P @ Zm.T + np.diag(Hd), Zm @ T @ P @ Zm.T])
            assert np.abs(r["acov"][b] - want).max() <= BAR * np.abs(want[0]).max()
            plain += 1
    assert plain >= 1


@pytest.mark.parametrize("name", ["rbc", "sw16_hp", "sw17_band", "wide33_16", "wide40_32", "sw64"])
def test_any_gain_is_the_circular_filter_in_the_time_domain(name):
    kw = cases.case(name)
    N, L = kw["n_grid"], kw["n_lags"]
    r = _reference(kw, correlation=False, spectrum=False)
    g = np.ones(N // 2 + 1) if kw["gain"] is None else kw["gain"]
    full = np.concatenate([g, g[-2:0:-1]])  # the gain on the whole grid, symmetric
    ang = 2.0 * np.pi * np.outer(np.arange(N), np.arange(N)) / N
    w = (np.sqrt(full)[None, :] * np.cos(ang)).sum(axis=1) / N  # real: the gain is symmetric
    v = np.array([np.dot(w, np.roll(w, d)) for d in range(N)])  # v[d] = sum_a w_a w_{a-d}
    for b in range(cases.NB):
        G = _folded_autocovariances(*_draw_inputs(kw, b), N)
        want = np.stack([sum(v[d] * G[(j - d) % N] for d in range(N)) for j in range(L + 1)])
        assert np.abs(r["acov"][b] - want).max() <= BAR * np.abs(want[0]).max()


@pytest.mark.parametrize("name", ["sw16_hp", "sw17_band", "sw49_dense", "nk_persistent"])
def test_the_spectrum_at_the_two_real_frequencies(name):
    kw = cases.case(name)
    r = _reference(kw, spectrum=True)
    nf = kw["n_grid"] // 2 + 1
    for b in range(cases.NB):
        T, R, Q, Zm, Hd = _draw_inputs(kw, b)
        scale = np.abs(r["spectrum"][b]).max()
        for n, sign in ((0, 1.0), (nf - 1, -1.0)):
            H = Zm @ np.linalg.solve(np.eye(T.shape[0]) - sign * T, R)
            want = (H @ Q @ H.T + np.diag(Hd)) / (2.0 * np.pi)
            assert np.abs(r["spectrum"][b, n] - want).max() <= BAR * scale


@pytest.mark.parametrize("name", ["sw16_hp", "sw40_hp", "nk_persistent"])
def test_the_hp_grid_at_512_against_2048(name):
    kw = cases.case(name)
    a, b = (_reference(kw, n_grid=N, n_lags=4, gain=batched.hp_gain(N), correlation=False, spectrum=False)["acov"] for N in (512, 2048))
    assert np.abs(a - b).max() <= BAR * np.abs(b).max()
