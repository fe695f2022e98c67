"""The numpy reference of the stochastic simulation at an occasionally binding bound (tests/constrained_sim_reference.py) against
independent formulations (CPU): period 0 of the perfect-foresight reference re-run every period, the table form the device kernels
use, time consistency with the perfect-foresight path, and the plain simulation where nothing binds.  Bar: 1e-10 of max|x|, the bar
of tests/test_constrained_reference.py.  The conditions every accuracy case of tests/constrained_sim_cases.py must meet -- from the
reference alone -- are asserted here and again, per case, by the GPU tests."""
import numpy as np
import pytest

from tests import anticipated_reference as aref
from tests import constrained_reference as cref
from tests import constrained_sim_cases as sc
from tests import constrained_sim_reference as ref

BAR = 1e-10


def check_conditions(name):
    """The conditions of an accuracy case, by the reference alone; returns its figures."""
    c, r = sc.case(name), sc.reference(name)
    assert name in sc.ACCURACY
    diag = min(np.diag(r["Mz"][b]).min() for b in range(sc.NB))
    margin = r["margin"].min()
    assert diag > 0.0
    assert (r["cond"] <= sc.COND_BAR).all()
    assert (r["cond_S"] <= sc.COND_S_BAR).all()
    assert margin >= sc.MARGIN_BAR
    assert ((r["path_status"] & ~ref.HORIZON_SHORT) == 0).all() and (r["fail_step"] == -1).all()
    assert bool((r["path_status"] & ref.HORIZON_SHORT).any()) == c["short"]
    return dict(diag=diag, cond=r["cond"].max(), cond_S=r["cond_S"].max(), margin=margin, iters=int(r["iters"].max()),
                duration=int(r["duration"].max()))


@pytest.mark.parametrize("name", sc.ACCURACY)
def test_every_case_meets_the_conditions(name):
    f = check_conditions(name)
    print(f"{name}: min diag(Mz) {f['diag']:.2e}, cond(M) <= {f['cond']:.1e}, cond(Mz[S,S]) <= {f['cond_S']:.1e}, smallest decision "
          f"quantity {f['margin']:.1e} max|q|, iters <= {f['iters']}, duration <= {f['duration']}")


def _longest_run(flags):
    best = cur = 0
    for v in flags:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


def test_the_cases_cover_what_they_must():
    R = {n: sc.reference(n) for n in sc.ACCURACY}
    spec = [sc.CASES[n] for n in sc.ACCURACY]
    case = [sc.case(n) for n in sc.ACCURACY]
    assert any(not r["S"].any() for r in R.values())                                        # a bound that never binds
    assert any((r["shadow"][:, :, 0] > 0.0).any() for r in R.values())                     # binding at t = 0
    assert any(_longest_run(row > 0.0) >= 4 for r in R.values() for row in r["shadow"].reshape(-1, r["shadow"].shape[-1]))
    assert any(r["duration"].max() >= 8 for r in R.values())
    assert any(r["iters"].max() >= 3 for r in R.values())
    assert any(s.get("short") for s in spec)
    assert {1, 2, 17, 32, 33, 64} <= {s["H"] for s in spec}
    assert {8, 17, 24, 40, 64} <= {c["n"] for c in case}
    assert {1, 5, 17} <= {s["n_paths"] for s in spec}
    assert any(s["n_shock"] < s["n_steps"] for s in spec) and any(s["n_shock"] == s["n_steps"] for s in spec)
    assert any(s["H"] > s["n_steps"] for s in spec) and any(s["H"] < s["n_steps"] for s in spec)
    assert any(c["shock"] == 0 for c in case) and any(c["shock"] == c["k"] - 1 > 0 for c in case)
    assert any(s["shared"] for s in spec) and any(not s["shared"] for s in spec)
    assert any(c["p"] == 0 for c in case) and any(c["p"] > 0 and c["d"] is not None for c in case)
    assert any(c["p"] > 0 and c["d"] is None for c in case)
    assert {None, "draw", "path"} <= {s["x0"] for s in spec}
    # the failure case fails, in some period after the first
    f = sc.reference("nk_fails")
    assert (f["path_status"] & ref.NO_REGIME).any() and (f["path_status"] == 0).any() and f["fail_step"].max() > 0


@pytest.mark.parametrize("name", ["rbc_h8", "sw17_h17", "nk_h17", "sw40_h32", "sw64_h64"])
def test_every_period_is_period_0_of_the_perfect_foresight_reference(name):
    """x[t] = period 0 of ``constrained_paths(eps = eps[t] alone, x0 = x[t-1], n_steps = H)``, with its nu, iters and status."""
    c, r = sc.case(name), sc.reference(name)
    H, worst = c["horizon"], 0.0
    for b in range(sc.NB):
        j = int(np.argmax((r["shadow"][b] > 0.0).sum(axis=-1)))  # the draw's path with the most binding periods
        prev = c["X0"][b, j]
        for t in range(c["n_steps"]):
            e = c["E"][b, j, t:t + 1] if t < c["n_shock"] else np.zeros((1, c["k"]))
            pf = cref.constrained_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], e, c["Cr"][b], c["Bd"][b], c["shock"], H, H, prev)
            assert (pf["status"] & ~cref.BEYOND_HORIZON) == 0 and pf["iters"] == r["iters"][b, j, t]
            assert (pf["nu"] == r["plan"][b, j, t]).all() and int(pf["S"].sum()) == r["duration"][b, j, t]
            worst = max(worst, np.abs(pf["x"][0] - r["x"][b, j, t]).max() / np.abs(r["x"][b]).max())
            prev = r["x"][b, j, t]
    print(f"{name}: period 0 of the perfect-foresight reference differs by {worst:.2e} of max|x|")
    assert worst <= BAR


@pytest.mark.parametrize("name", sc.ACCURACY)
def test_the_table_form_gives_the_same_path(name):
    """xu = T x[t-1] + R eps[t], q = Cq xu - bound, x[t] = xu + W nu with Cq[h] = c'T^h and W[:, j] = G^j R[:, s]: the algebra of
    the device kernels."""
    c, r = sc.case(name), sc.reference(name)
    H, worst, worst_q = c["horizon"], 0.0, 0.0
    for b in range(sc.NB):
        G, _ = aref.gain(c["B"][b], c["C"][b], c["T"][b])
        Cq, W = ref.tables(G, c["T"][b], c["R"][b], c["Cr"][b], c["shock"], H)
        for j in range(c["n_paths"]):
            x = c["X0"][b, j]
            for t in range(c["n_steps"]):
                xu = c["T"][b] @ x + (c["R"][b] @ c["E"][b, j, t] if t < c["n_shock"] else 0.0)
                q = Cq @ xu - c["Bd"][b]
                it = cref.regime_iteration(r["Mz"][b], q)
                assert it["status"] == 0 and it["iters"] == r["iters"][b, j, t] and (it["S"] == r["S"][b, j, t]).all()
                x = xu + W @ it["nu"]
                worst = max(worst, np.abs(x - r["x"][b, j, t]).max() / np.abs(r["x"][b]).max())
                worst_q = max(worst_q, np.abs(q - r["q"][b, j, t]).max() / r["qmax"][b, j, t])
    print(f"{name}: the table form differs by {worst:.2e} of max|x|, its q by {worst_q:.2e} of max|q|")
    assert worst <= BAR and worst_q <= BAR


@pytest.mark.parametrize("name", sc.TIME_CONSISTENCY)
def test_replanning_every_period_reproduces_the_perfect_foresight_path(name):
    """Shocks at t = 0 only: nothing new arrives afterwards, so re-planning every period changes no plan, and the simulated path is
    the perfect-foresight path of tests/constrained_reference.py -- on paths where that path does not violate the bound beyond
    its horizon."""
    assert {sc.CASES[n]["model"] for n in sc.TIME_CONSISTENCY} >= {"rbc", "sw17", "sw40", "sw64"}
    c, r = sc.case(name), sc.reference(name)
    assert c["n_shock"] == 1 and c["n_steps"] == 2 * c["horizon"]
    worst, used, bound_periods = 0.0, 0, 0
    for b in range(sc.NB):
        for j in range(c["n_paths"]):
            pf = cref.constrained_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], c["E"][b, j], c["Cr"][b], c["Bd"][b], c["shock"],
                                        c["horizon"], c["n_steps"], c["X0"][b, j])
            if pf["status"] != 0:
                continue
            used += 1
            bound_periods += int(pf["S"].sum())
            worst = max(worst, np.abs(pf["x"] - r["x"][b, j]).max() / np.abs(r["x"][b]).max())
    print(f"{name}: {used} paths, {bound_periods} binding periods, re-planned against perfect foresight {worst:.2e} of max|x|")
    assert used > 0 and bound_periods > 0 and worst <= BAR


def test_a_bound_that_never_binds_gives_the_plain_simulation():
    c, r = sc.case("rbc_none"), sc.reference("rbc_none")
    assert (r["shadow"] == 0.0).all() and (r["plan"] == 0.0).all() and (r["duration"] == 0).all() and (r["iters"] == 1).all()
    for b in range(sc.NB):
        w = np.zeros((c["n_steps"], c["n"]))
        w[:c["n_shock"]] = c["E"][b, 0] @ c["R"][b].T
        assert (aref.propagate(c["T"][b], w) == r["x"][b, 0]).all()
