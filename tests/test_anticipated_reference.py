"""The numpy reference of the anticipated-shock paths (tests/anticipated_reference.py) against independent formulations (CPU):
the stacked-time solve of the model equations (the reference project's perfect-foresight formulation, for the linearised model),
superposition over arrival dates (news), and two degenerate cases.  Bar: 1e-10 of max|x|."""
import numpy as np
import pytest

from tests import anticipated_cases as ac
from tests import anticipated_reference as ref

BAR = 1e-10
PF = sorted(n for n, s in ac.CASES.items() if s["mode"] == "perfect_foresight")
NEWS = sorted(n for n, s in ac.CASES.items() if s["mode"] == "news")


def _stacked_time(A, B, C, D, T, eps, x0, horizon):
    """x[0 .. horizon-1] from the block-tridiagonal system  A x[t-1] + B x[t] + C x[t+1] + D eps[t] = 0,  t < horizon, closed by
    x[horizon] = T x[horizon-1] (no shock at or after ``horizon``): the last diagonal block is B + C T."""
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
    return np.linalg.solve(big, rhs).reshape(horizon, n)


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_anticipation_matters_and_the_solve_is_well_conditioned(name):
    r = ac.reference(name)
    print(f"{name}: max_j |G^j R| / |R| >= {r['relevance'].min():.3f}, cond(M) <= {r['cond'].max():.1e}")
    assert (r["relevance"] >= ac.RELEVANCE).all() and (r["cond"] <= ac.COND_BAR).all()


@pytest.mark.parametrize("name", PF)
def test_perfect_foresight_against_the_stacked_time_solve(name):
    c, r = ac.case(name), ac.reference(name)
    worst = 0.0
    for b in range(ac.NB):
        M = c["B"][b] + c["C"][b] @ c["T"][b]
        A = -M @ c["T"][b]
        assert np.abs(M @ c["R"][b] + c["D"][b]).max() <= 1e-12 * np.abs(c["D"][b]).max()  # R is the model's R
        s = c["n_paths"] - 1
        horizon = max(c["n_steps"], c["n_shock"])
        x = _stacked_time(A, c["B"][b], c["C"][b], c["D"][b], c["T"][b], c["E"][b, s], c["X0"][b, s], horizon)[:c["n_steps"]]
        worst = max(worst, np.abs(x - r["x"][b, s]).max() / np.abs(r["x"][b]).max())
    print(f"{name}: stacked-time solve differs by {worst:.2e} of max|x|")
    assert worst <= BAR


@pytest.mark.parametrize("name", NEWS)
def test_news_is_the_superposition_of_perfect_foresight_paths(name):
    """What is learnt at ``a`` about the shocks of ``a .. a + L`` is a perfect-foresight path started at ``a``; the expected shocks
    are made from arrivals ``nu`` by ``expected_shocks_from_news``, and the news path is the sum over ``a``."""
    from geconpy_amd import batched

    c = ac.case(name)
    n_steps, S = c["n_steps"], c["n_shock"]
    worst = 0.0
    for b in range(ac.NB):
        nu = c["E"][b, 0].copy()  # any array of this shape serves as arrivals ...
        for t in range(S):
            nu[t, max(S - t, 0):] = 0.0  # ... about shocks before period S: later periods have e = 0 by the entry's definition
        e =batched.expected_shocks_from_news(nu)
        got = ref.anticipated_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], e, n_steps, "news", c["X0"][b, 0])["x"]
        G, _ = ref.gain(c["B"][b], c["C"][b], c["T"][b])
        total = ref.propagate(c["T"][b], np.zeros((n_steps, c["n"])), c["X0"][b, 0])  # the path of x0 alone
        for a in range(S):
            w = ref.anticipation(G, c["R"][b], nu[a], n_steps + nu.shape[0], "perfect_foresight")  # w of the path started at a
            total[a:] += ref.propagate(c["T"][b], w[:n_steps - a])
        worst = max(worst, np.abs(total - got).max() / np.abs(got).max())
    print(f"{name}: superposition differs by {worst:.2e} of max|x|")
    assert worst <= BAR


def test_expected_shocks_from_news_against_the_triple_loop():
    from geconpy_amd import batched

    rng = np.random.default_rng(3)
    for shape in ((5, 3, 2), (2, 6, 1), (7, 1, 3), (1, 1, 1)):
        nu = rng.standard_normal(shape)
        assert np.abs(batched.expected_shocks_from_news(nu) - ref.triple_loop_expected_shocks(nu)).max() <= 1e-14
    nu = rng.standard_normal((2, 3, 5, 4, 2))  # leading axes (draws, paths) pass through
    e = batched.expected_shocks_from_news(nu)
    assert np.abs(e[1, 2] - ref.triple_loop_expected_shocks(nu[1, 2])).max() <= 1e-14


@pytest.mark.parametrize("name", ["rbc_pf", "nk_pf", "sw40_pf"])
def test_a_shock_at_t0_alone_is_the_impulse_response(name):
    c = ac.case(name)
    for b in range(ac.NB):
        eps = np.zeros((c["n_shock"], c["k"]))
        eps[0] = c["E"][b, 0, 0]
        x = ref.anticipated_paths(c["B"][b], c["C"][b], c["T"][b], c["R"][b], eps, c["n_steps"])["x"]
        irf, cur = np.empty_like(x), c["R"][b] @ eps[0]
        for h in range(c["n_steps"]):
            irf[h] = cur
            cur = c["T"][b] @ cur
        assert np.abs(x - irf).max() <= BAR * np.abs(irf).max()


def test_news_without_a_lead_is_simulate():
    c, r = ac.case("sw17_news0"), ac.reference("sw17_news0")
    assert c["n_lead"] == 0
    x = np.empty_like(r["x"])
    prev = c["X0"].copy()
    for t in range(c["n_steps"]):
        prev = np.einsum("bij,bsj->bsi", c["T"], prev) + np.einsum("bij,bsj->bsi", c["R"], c["E"][:, :, t, 0])
        x[:, :, t] = prev
    assert np.abs(x - r["x"]).max() <= BAR * np.abs(x).max()
