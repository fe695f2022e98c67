"""The numpy reference of the conditional forecast (tests/conditional_forecast_reference.py) against three independent
formulations, without a GPU: (1) a covariance-form Kalman filter and Rauch-Tung-Striebel smoother run over the horizon from the
known x0 with the conditions as noiseless observations (e+ = 0, all shocks free, diagonal and full Q); (2) the period-by-period
solve for the controlled shocks in the square case; (3) np.linalg.lstsq on the system scaled by Qt^(1/2).  The bar between two
references is 1e-10 of max|x|; every case asserts cond_2(G) <= 1e5 from the reference alone."""
import numpy as np
import pytest

from tests import conditional_forecast_cases as cc
from tests import conditional_forecast_reference as ref

BAR = 1e-10


def _draws(name):
    """(case, per draw b: the arguments of ref.conditional_forecast for path 0)."""
    c = cc.case(name)
    return c, [dict(T=c["T"][b], R=c["R"][b], Q=c["Qf"][b], Z=c["Z"], d=c["d"], x0=c["X0"][b, 0], cond_t=c["cond_t"], cond_j=c["cond_j"],
                    cond_val=c["V"][b, 0], n_steps=c["n_steps"]) for b in range(cc.NB)]


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_every_case_is_well_conditioned_and_meets_its_conditions(name):
    c, r = cc.case(name), cc.reference(name)
    print(f"{name}: cond_2(G) per draw {r['cond']}")
    assert (r["cond"] <= cc.COND_BAR).all()
    scale = np.abs(r["x"]).max(axis=(1, 2, 3))
    got = r["observed"][:, :, c["cond_t"], c["cond_j"]]
    assert (np.abs(got - c["V"]).max(axis=(1, 2)) <= BAR * scale).all()
    if c["free"] is not None and c["E"] is not None:  # the shocks that are not free are the baseline's
        fixed = [j for j in range(c["k"]) if j not in c["free"]]
        n_sh = c["E"].shape[2]
        assert np.array_equal(r["shocks"][:, :, :n_sh, fixed], c["E"][..., fixed])


def kalman_rts_mean(T, R, Q, Z, d, x0, cond_t, cond_j, cond_val, n_steps):
    """The smoothed mean of x[0 .. n_steps-1] given x[-1] = x0 exactly and the noiseless observations
    d[j] + Z[j] x[t] = v: covariance-form filter forward, RTS backward (pseudo-inverse of the singular predicted covariance)."""
    m = T.shape[0]
    d = np.zeros(Z.shape[0]) if d is None else d
    RQR = R @ Q @ R.T
    a, P = np.asarray(x0, dtype=float), np.zeros((m, m))
    ap, Pp, af, Pf = [], [], [], []
    for t in range(n_steps):
        a, P = T @ a, T @ P @ T.T + RQR
        ap.append(a)
        Pp.append(P)
        rows = [c for c in range(len(cond_t)) if cond_t[c] == t]
        if rows:
            Zc = Z[[cond_j[c] for c in rows]]
            v = np.array([cond_val[c] - d[cond_j[c]] for c in rows]) - Zc @ a
            K = np.linalg.solve(Zc @ P @ Zc.T, Zc @ P).T
            a, P = a + K @ v, P - K @ Zc @ P
            P = 0.5 * (P + P.T)
        af.append(a)
        Pf.append(P)
    xs = [None] * n_steps
    xs[-1] = af[-1]
    for t in range(n_steps - 2, -1, -1):
        J = Pf[t] @ T.T @ np.linalg.pinv(Pp[t + 1], rcond=1e-13, hermitian=True)
        xs[t] = af[t] + J @ (xs[t + 1] - ap[t + 1])
    return np.stack(xs)


@pytest.mark.parametrize("name", ["sw16_paths", "sw17_gap", "sw40_last", "sw49_dense", "sw64_p16", "sw96"])  # diagonal and full Q
def test_mean_equals_kalman_filter_and_rts_smoother_from_a_known_state(name):
    c, draws = _draws(name)
    assert c["free"] is None
    for b, a in enumerate(draws):
        r = ref.conditional_forecast(**a)  # e+ = 0: the mean
        assert np.linalg.cond(r["G"]) <= cc.COND_BAR
        x = kalman_rts_mean(**a)
        err = np.abs(x - r["x"]).max() / np.abs(r["x"]).max()
        print(f"{name} draw {b}: Kalman + RTS against the reference {err:.1e} of max|x|")
        assert err <= BAR


@pytest.mark.parametrize("name", ["rbc_square", "sw17_square", "sw40_square64"])
def test_square_case_equals_the_period_by_period_solve(name):
    c, draws = _draws(name)
    F = list(range(c["k"])) if c["free"] is None else sorted(c["free"])
    for b, a in enumerate(draws):
        eps = None if c["E"] is None else c["E"][b, 0]
        r = ref.conditional_forecast(**a, eps=eps, free=F)
        assert np.linalg.cond(r["G"]) <= cc.COND_BAR
        T, R, Z, d = a["T"], a["R"], a["Z"], np.zeros(c["p"]) if a["d"] is None else a["d"]
        e = np.zeros((a["n_steps"], c["k"]))
        if eps is not None:
            e[:len(eps)] = eps
        x, xs = a["x0"], []
        for t in range(a["n_steps"]):
            rows = [i for i in range(len(a["cond_t"])) if a["cond_t"][i] == t]
            if rows:
                J = [a["cond_j"][i] for i in rows]
                assert len(J) == len(F)
                want = np.array([a["cond_val"][i] for i in rows]) - d[J] - Z[J] @ (T @ x + R @ e[t])
                e[t, F] += np.linalg.solve(Z[J] @ R[:, F], want)
            x = T @ x + R @ e[t]
            xs.append(x)
        err = np.abs(np.stack(xs) - r["x"]).max() / np.abs(r["x"]).max()
        err_e = np.abs(e - r["shocks"]).max() / np.abs(r["shocks"]).max()
        print(f"{name} draw {b}: period by period against the reference {err:.1e} of max|x|, shocks {err_e:.1e}")
        assert err <= BAR


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_correction_equals_least_squares_on_the_scaled_system(name):
    c, draws = _draws(name)
    F = list(range(c["k"])) if c["free"] is None else sorted(c["free"])
    for b, a in enumerate(draws):
        eps = None if c["E"] is None else c["E"][b, 0]
        r = ref.conditional_forecast(**a, eps=eps, free=F)
        W, Qt = ref.system(a["T"], a["R"], a["Q"], a["Z"], a["cond_t"], a["cond_j"], F)
        S = np.linalg.cholesky(Qt)  # Delta = S u with u of minimum 2-norm: the minimum Qt^-1 norm
        base = np.zeros((a["n_steps"], c["k"]))
        if eps is not None:
            base[:len(eps)] = eps
        d = np.zeros(c["p"]) if a["d"] is None else a["d"]
        xb = ref.simulate(a["T"], a["R"], base, a["x0"])
        rhs = np.array([v - d[j] - a["Z"][j] @ xb[t] for t, j, v in zip(a["cond_t"], a["cond_j"], a["cond_val"])])
        u = np.linalg.lstsq(W @ S, rhs, rcond=None)[0]
        e = base.copy()
        e[:W.shape[1] // len(F), F] += (S @ u).reshape(-1, len(F))
        x = ref.simulate(a["T"], a["R"], e, a["x0"])
        err = np.abs(x - r["x"]).max() / np.abs(r["x"]).max()
        print(f"{name} draw {b}: scaled least squares against the reference {err:.1e} of max|x|")
        assert err <= BAR


def test_no_conditions_is_the_plain_simulation():
    c = cc.case("sw17_subset")
    r = ref.conditional_forecast(c["T"][0], c["R"][0], c["Qf"][0], c["Z"], c["d"], c["X0"][0, 0], [], [], [], c["n_steps"], eps=c["E"][0, 0])
    assert np.array_equal(r["x"], ref.simulate(c["T"][0], c["R"][0], c["E"][0, 0], c["X0"][0, 0]))
