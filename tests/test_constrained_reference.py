"""The numpy reference of the paths under an occasionally binding bound (tests/constrained_reference.py) against independent
formulations (CPU): the regime-switched stacked-time system, brute force over all binding sets, the unconstrained path, and a
configuration without a regime.  Bar: 1e-10 of max|x|, the bar of tests/test_anticipated_reference.py.  The conditions every
accuracy case of tests/constrained_cases.py must meet -- from the reference alone -- are asserted here and again, per case, by the
GPU tests."""
import itertools

import numpy as np
import pytest

from tests import anticipated_cases as ac
from tests import anticipated_reference as aref
from tests import constrained_cases as cc
from tests import constrained_reference as ref

BAR = 1e-10
UNIT = sorted(n for n, s in cc.CASES.items() if s.get("unit"))


def check_conditions(name):
    """The conditions of an accuracy case, by the reference alone; returns its figures."""
    c, r = cc.case(name), cc.reference(name)
    H = c["horizon"]
    diag = min(np.diag(r["Mz"][b]).min() for b in range(cc.NB))
    margin = (r["margin"] / r["qmax"]).min()
    beyond = (r["gap"][:, :, H:] / r["qmax"][:, :, None]).min() if c["n_steps"] > H else np.inf
    assert diag > 0.0
    assert (r["cond"] <= cc.COND_BAR).all() and (r["cond_S"] <= cc.COND_BAR).all()
    assert margin >= cc.MARGIN_BAR
    if c["beyond"]:
        assert beyond < -cc.MARGIN_BAR and (r["path_status"] & ref.BEYOND_HORIZON).any()
        assert ((r["path_status"] & ~ref.BEYOND_HORIZON) == 0).all()
    else:
        assert beyond >= cc.MARGIN_BAR and (r["path_status"] == 0).all()
    return dict(diag=diag, cond=r["cond"].max(), cond_S=r["cond_S"].max(), margin=margin, beyond=beyond, iters=int(r["iters"].max()))


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_every_case_meets_the_conditions(name):
    f = check_conditions(name)
    print(f"{name}: min diag(Mz) {f['diag']:.2e}, cond(M) <= {f['cond']:.1e}, cond(Mz[S,S]) <= {f['cond_S']:.1e}, smallest decision "
          f"quantity {f['margin']:.1e} max|q|, gap beyond H >= {f['beyond']:.1e} max|q|, iters <= {f['iters']}")


def test_the_cases_cover_what_they_must():
    S = {n: cc.reference(n)["S"] for n in cc.CASES}
    spec = cc.CASES.values()
    assert any(not S[n].any() for n in S)                                                  # no binding period
    assert any(S[n][:, :, 0].any() for n in S)                                             # binding at t = 0
    assert any(cc.spells(row) >= 2 for n in S for row in S[n].reshape(-1, S[n].shape[-1]))  # two separate spells
    assert any(S[n].all(axis=-1).any() for n in S)                                         # every period binds
    assert cc.reference("nk_iters")["iters"].max() >= 3
    assert {1, 2, 17, 32, 33, 64} <= {s["H"] for s in spec}
    assert {8, 17, 24, 40, 64} <= {cc.case(n)["n"] for n in cc.CASES}
    assert {1, 5, 17} <= {s["n_paths"] for s in spec}
    assert any(s["n_steps"] == s["H"] for s in spec) and any(s["n_steps"] > s["H"] for s in spec)
    assert any(s["n_shock"] < s["H"] for s in spec) and any(s["n_shock"] == s["H"] for s in spec)
    assert any(s["n_shock"] > s["n_steps"] for s in spec)
    assert any(cc.case(n)["shock"] == 0 for n in cc.CASES) and any(cc.case(n)["shock"] == cc.case(n)["k"] - 1 > 0 for n in cc.CASES)
    assert any(s["shared"] and S[n].any() for n, s in cc.CASES.items()) and any(not s["shared"] for s in spec)
    assert any(cc.case(n)["p"] == 0 for n in cc.CASES) and any(cc.case(n)["p"] > 0 for n in cc.CASES)
    assert any(s.get("beyond") for s in spec)


def _stacked_time_with_regimes(A, B, C, D, T, eps, x0, horizon, c, bound, eq, binding):
    """x[0 .. horizon-1] of  A x[t-1] + B x[t] + C x[t+1] + D eps[t] = 0, closed by x[horizon] = T x[horizon-1], where equation ``eq``
    of every period in ``binding`` is replaced by  c'x[t] = bound."""
    n = A.shape[0]
    big, rhs = np.zeros((horizon * n, horizon * n)), np.zeros(horizon * n)
    for t in range(horizon):
        rows = slice(t * n, (t + 1) * n)
        big[rows, rows] = B + (C @ T if t == horizon - 1 else 0.0)
        if t > 0:
            big[rows, (t - 1) * n:t * n] = A
        if t + 1 < horizon:
            big[rows, (t + 1) * n:(t + 2) * n] = C
        rhs[rows] = -(D @ eps[t] if t < len(eps) else 0.0) - (A @ x0 if t == 0 else 0.0)
        if t in binding:
            big[t * n + eq] = 0.0
            big[t * n + eq, rows] = c
            rhs[t * n + eq] = bound
    return np.linalg.solve(big, rhs).reshape(horizon, n)


@pytest.mark.parametrize("name", UNIT)
def test_the_regime_switched_stacked_time_system_gives_the_same_path(name):
    """With D[:, s] = e_i the shadow shock enters equation i alone: choosing it is replacing that equation, in the binding periods,
    by the bound holding with equality."""
    assert {cc.CASES[n]["model"] for n in UNIT} >= {"rbc", "sw17", "sw40", "sw64"} and cc.CASES["sw64_h64"]["H"] == 64
    c, r = cc.case(name), cc.reference(name)
    s, worst, bound_periods = c["shock"], 0.0, 0
    for b in range(cc.NB):
        eq = int(np.flatnonzero(c["D"][b][:, s])[0])
        assert (c["D"][b][:, s] == np.eye(c["n"])[eq]).all()
        M = c["B"][b] + c["C"][b] @ c["T"][b]
        assert np.abs(M @ c["R"][b] + c["D"][b]).max() <= 1e-12
        for j in (int(np.argmax(r["S"][b].sum(axis=-1))),):  # the draw's path with the most binding periods
            binding = set(np.flatnonzero(r["S"][b, j]).tolist())
            bound_periods += len(binding)
            horizon = max(c["n_steps"], c["n_shock"])
            x = _stacked_time_with_regimes(-M @ c["T"][b], c["B"][b], c["C"][b], c["D"][b], c["T"][b], c["E"][b, j], c["X0"][b, j], horizon,
                                           c["Cr"][b], c["Bd"][b], eq, binding)[:c["n_steps"]]
            worst = max(worst, np.abs(x - r["x"][b, j]).max() / np.abs(r["x"][b]).max())
    print(f"{name}: the regime-switched stacked-time solve ({bound_periods} binding periods) differs by {worst:.2e} of max|x|")
    assert bound_periods > 0 and worst <= BAR


def _minors_positive(Mz):
    H = Mz.shape[0]
    return all(np.linalg.det(Mz[np.ix_(idx, idx)]) > 0.0 for size in range(1, H + 1) for idx in itertools.combinations(range(H), size))


def _brute_force(Mz, q):
    """Every binding set S whose solution satisfies nu[S] > 0 and gap >= 0 off S."""
    H = q.shape[0]
    found = []
    for bits in range(1 << H):
        S = np.array([(bits >> h) & 1 for h in range(H)], bool)
        nu = np.zeros(H)
        if S.any():
            nu[S] = np.linalg.solve(Mz[np.ix_(S, S)], -q[S])
        gap = q + Mz @ nu
        if (nu[S] > 0.0).all() and (gap[~S] >= 0.0).all():
            found.append(S)
    return found


@pytest.mark.parametrize("model, shock, H", [("rbc", 0, 8), ("sw17", 0, 8), ("sw40", 6, 7), ("sw64", 7, 8)])
def test_brute_force_over_all_binding_sets_finds_the_same_one(model, shock, H):
    mdl = ac.model(model)
    rng = np.random.default_rng([41, *model.encode()])
    n, k = mdl["R"].shape[1:]
    bound_periods = 0
    for b in range(cc.NB):
        var = int(np.argmax(np.abs(mdl["R"][b][:, shock])))
        c = np.zeros(n)
        c[var] = np.sign(mdl["R"][b][var, shock])
        G, _ = aref.gain(mdl["B"][b], mdl["C"][b], mdl["T"][b])
        Mz = ref.shadow_matrix(G, mdl["T"][b], mdl["R"][b], c, shock, H)
        assert _minors_positive(Mz)
        for _ in range(3):
            eps = 0.01 * rng.standard_normal((H, k))
            cx = aref.anticipated_paths(mdl["B"][b], mdl["C"][b], mdl["T"][b], mdl["R"][b], eps, H)["x"] @ c
            r = ref.constrained_paths(mdl["B"][b], mdl["C"][b], mdl["T"][b], mdl["R"][b], eps, c, 0.5 * cx.min(), shock, H, H)
            assert r["status"] == 0 and r["margin"] >= cc.MARGIN_BAR * np.abs(r["q"]).max()
            found = _brute_force(Mz, r["q"])
            assert len(found) == 1 and (found[0] == r["S"]).all()
            bound_periods += int(r["S"].sum())
            # the complementarity conditions, on the path itself
            assert (r["nu"] >= 0.0).all() and (r["gap"][:H] >= -1e-12 * np.abs(r["q"]).max()).all()
            assert np.abs(r["nu"] * r["gap"][:H]).sum() <= 1e-12 * np.abs(r["nu"]).max() * np.abs(r["q"]).max()
    assert bound_periods > 0


def test_without_a_binding_period_the_path_is_the_unconstrained_one():
    c, r = cc.case("rbc_none"), cc.reference("rbc_none")
    assert not r["S"].any() and (r["iters"] == 1).all() and (r["nu"] == 0.0).all()
    for b in range(cc.NB):
        u = aref.anticipated_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], c["E"][b, 0], c["n_steps"], "perfect_foresight", c["X0"][b, 0])
        assert (u["x"] == r["x"][b, 0]).all() and (u["w"] == r["w"][b, 0]).all()


def test_a_matrix_that_is_not_a_p_matrix_can_leave_no_regime():
    """full_nk, shock 2, the third-most-moved variable, draw 1: Mz at H = 8 has a non-positive principal minor, and with 64
    iterations allowed the regime iteration cycles on some paths."""
    mdl, b, shock, H = ac.model("full_nk"), 1, 2, 8
    n, k = mdl["R"].shape[1:]
    var = int(np.argsort(-np.abs(mdl["R"][b][:, shock]))[2])
    c = np.zeros(n)
    c[var] = np.sign(mdl["R"][b][var, shock])
    G, _ = aref.gain(mdl["B"][b], mdl["C"][b], mdl["T"][b])
    assert not _minors_positive(ref.shadow_matrix(G, mdl["T"][b], mdl["R"][b], c, shock, H))
    rng = np.random.default_rng(43)
    statuses = []
    for _ in range(20):
        eps = 0.01 * rng.standard_normal((H, k))
        cx = aref.anticipated_paths(mdl["B"][b], mdl["C"][b], mdl["T"][b], mdl["R"][b], eps, H)["x"] @ c
        r = ref.constrained_paths(mdl["B"][b], mdl["C"][b], mdl["T"][b], mdl["R"][b], eps, c, 0.5 * cx.min(), shock, H, H, max_iter=64)
        statuses.append(r["status"])
        if r["status"] == ref.NO_REGIME:
            assert r["iters"] == 64 and np.isnan(r["x"]).all() and np.isnan(r["nu"]).all()
    assert ref.NO_REGIME in statuses
