"""GPU: the anticipated-shock paths (dsge_anticipated_paths_batched; csrc/dsge_anticipated.hpp) against the numpy reference of
tests/anticipated_reference.py (np.linalg.solve for G, then the recursions; held to the stacked-time solve and to superposition at
1e-10 by tests/test_anticipated_reference.py).

Bar: the project's 1e-9, per output block and draw, on error / max|x| of the draw's reference paths -- no floor at 1; G at 1e-9 of
max|G|.  Every accuracy case has max_j |G^j R| / |R| >= 0.05 and cond_2(M) <= 1e5 by the reference alone, and prints its largest
error."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched

from tests import anticipated_cases as ac

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _run(c, **over):
    kw = {**ac.kwargs(c), "outputs": ac.outputs(c), **over}
    return batched.anticipated_paths_batched(c["B"], c["C"], c["T"], c["R"], c["eps"], **kw)


@pytest.fixture(scope="module")
def results():
    """The device result of every case, computed on first use and shared (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(ac.case(name))
        return cache[name]

    return get


def _scale(r):
    return np.abs(r["x"]).max(axis=(1, 2, 3))


# ---- parity: n = 8, 16, 17, 24, 40, 49, 64; k = 1, 8; 1, 16, 17 paths; n_steps = 1, 2, 40; n_shock_steps below, equal to and above
# ---- n_steps; n_lead = 0, 1, 5; shared / per-draw / per-path eps and x0, x0 NULL; selector and dense Z, d, p = 0 (the table of CASES)
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_parity_with_the_reference(results, name):
    c, r, got = ac.case(name), ac.reference(name), results(name)
    assert (r["relevance"] >= ac.RELEVANCE).all(), r["relevance"]
    assert (r["cond"] <= ac.COND_BAR).all(), r["cond"]
    assert (got["status"] == 0).all()
    scale = _scale(r)
    errs = {}
    for key in ("x", "w") + (("observed",) if c["p"] else ()):
        assert got[key].shape == r[key].shape, key
        errs[key] = max(np.abs(got[key][b] - r[key][b]).max() / scale[b] for b in range(ac.NB))
    errs["G"] = max(np.abs(got["G"][b] - r["G"][b]).max() / np.abs(r["G"][b]).max() for b in range(ac.NB))
    print(f"{name} (n = {c['n']}, k = {c['k']}, cond(M) <= {r['cond'].max():.1e}, |G^j R| / |R| >= {r['relevance'].min():.2f}):",
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_simulate_on_the_anticipation_term_reproduces_the_path(results, name):
    c, r, got = ac.case(name), ac.reference(name), results(name)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(c["n"]), (ac.NB, c["n"], c["n"])))
    sim = batched.simulate_batched(c["T"], eye, got["w"], x0=c["X0"])["paths"]
    gap = max(np.abs(sim[b] - got["x"][b]).max() / _scale(r)[b] for b in range(ac.NB))
    print(f"{name}: simulate(T, I, w_out) differs from x_out by {gap:.2e} of max|x|")
    assert gap <= BAR


@pytest.mark.parametrize("name", sorted(n for n, s in ac.CASES.items() if s["mode"] == "perfect_foresight" and s["n_steps"] > 1))
def test_the_model_equations_hold_along_the_perfect_foresight_path(results, name):
    """A x[t-1] + B x[t] + C x[t+1] + D eps[t] = 0 with A = -M T on the DEVICE path, for every t whose successor is inside it."""
    c, r, got = ac.case(name), ac.reference(name), results(name)
    worst = 0.0
    for b in range(ac.NB):
        M = c["B"][b] + c["C"][b] @ c["T"][b]
        A = -M @ c["T"][b]
        x = np.concatenate([c["X0"][b][:, None], got["x"][b]], axis=1)  # (n_paths, 1 + n_steps, n): x[-1] first
        e = np.zeros((c["n_paths"], c["n_steps"], c["k"]))
        n_e = min(c["n_steps"], c["n_shock"])
        e[:, :n_e] = c["E"][b][:, :n_e]
        res = x[:, :-2] @ A.T + x[:, 1:-1] @ c["B"][b].T + x[:, 2:] @ c["C"][b].T + e[:, :-1] @ c["D"][b].T
        worst = max(worst, np.abs(res).max() / (_scale(r)[b] * np.abs(M).max()))
    print(f"{name}: the model equations miss by {worst:.2e} of max|x| max|M|")
    assert worst <= BAR


@pytest.mark.parametrize("name", ["nk_pf", "sw40_news5"])
def test_two_calls_give_the_same_bits(results, name):
    again = _run(ac.case(name))
    for key in ("x", "w", "observed", "G", "status"):
        assert_array_equal(again[key], results(name)[key])


@pytest.mark.parametrize("name", ["rbc_beyond", "sw64_pf", "nk_news5"])
def test_any_subset_of_the_outputs_gives_the_same_bits(results, name):
    """x alone parks w in its own slabs, observed alone in library scratch, G alone runs the setup only."""
    c = ac.case(name)
    for outs in (("x",), ("w",), ("observed",), ("G",), ("x", "observed")):
        got = _run(c, outputs=outs)
        assert sorted(got) == sorted(outs + ("status",))
        for key in outs:
            assert_array_equal(got[key], results(name)[key])


def test_news_on_a_grid_past_the_wide_step_threshold_gives_the_same_bits(results):
    """Up to 512 workgroups news with a lead runs four periods per Horner step, beyond that one (launch_anticipated.hip).  The 17
    paths of sw40_news5 repeated 161 times make 3 x 172 = 516 workgroups, and every copy -- in other columns of other workgroups,
    through the other kernel -- must carry the bits of the small call."""
    c, small = ac.case("sw40_news5"), results("sw40_news5")
    reps = 161
    assert ac.NB * -(-17 * reps // 16) > 512 and c["n_paths"] == 17 and c["n_lead"] > 0
    eps = np.ascontiguousarray(np.tile(c["eps"], (1, reps, 1, 1, 1)))
    got = batched.anticipated_paths_batched(c["B"], c["C"], c["T"], c["R"], eps, **ac.kwargs(c), outputs=("x", "observed"))
    assert (got["status"] == 0).all()
    for key in ("x", "observed"):
        for i in (0, 1, 80, reps - 1):
            assert_array_equal(got[key][:, 17 * i:17 * (i + 1)], small[key])


# ---- failures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nk_pf", "sw40_news5"])
def test_a_failed_draw_between_two_healthy_ones(results, name):
    c = ac.case(name)
    status = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32)
    got = _run(c, status=status)
    assert got["status"].tolist() == [0, _lib.ST_NOT_CONVERGED, 0] and status.tolist() == [0, 1, 0]
    for key in ("x", "w", "observed", "G"):
        assert np.isnan(got[key][1]).all()
        assert_array_equal(got[key][[0, 2]], results(name)[key][[0, 2]])


@pytest.mark.parametrize("name, rank_tol", [("nk_pf", 0.0), ("sw16_news1", 0.0), ("sw17_pf", 0.0), ("sw64_pf", 1e-10)])
def test_a_singular_draw_gets_the_status_bit_and_does_not_touch_its_neighbours(results, name, rank_tol):
    """Row 2 of B of draw 1 is minus that row of C T: row 2 of M = B + C T is zero up to the rounding of the two products (the
    host's here, the device's there), which the elimination carries into the last pivot.  With the default rank_tol = 1e-14 that
    pivot, computed on the CPU by the same elimination, is <= 2e-16 max|M| on full_nk, sw16 and sw17 -- fifty times below the
    threshold -- but 2.7e-15 max|M| on sw64, so the n = 64 case passes rank_tol = 1e-10 (docs/design/anticipated_shocks.md)."""
    c = ac.case(name)
    B = c["B"].copy()
    B[1, 2] = -(c["C"][1] @ c["T"][1])[2]
    kw = {**ac.kwargs(c), "outputs": ac.outputs(c), "rank_tol": rank_tol}
    got = batched.anticipated_paths_batched(B, c["C"], c["T"], c["R"], c["eps"], **kw)
    assert got["status"].tolist() == [0, _lib.ST_ANTICIPATION_SINGULAR, 0] and _lib.ST_ANTICIPATION_SINGULAR == 2048
    for key in ac.outputs(c):
        assert np.isnan(got[key][1]).all() and np.isfinite(got[key][[0, 2]]).all()
        assert_array_equal(got[key][[0, 2]], results(name)[key][[0, 2]])


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nk_pf", "sw40_news5", "sw17_news0"])
def test_device_tensors_equal_the_host_twin(results, name):
    import torch
    from geconpy_amd.engine import LogpEngine

    c, eng = ac.case(name), LogpEngine(0)
    dev = lambda a: None if a is None else eng.to_device(a)  # noqa: E731
    kw = {key: dev(v) if isinstance(v, np.ndarray) else v for key, v in ac.kwargs(c).items()}
    got = eng.anticipated_paths(dev(c["B"]), dev(c["C"]), dev(c["T"]), dev(c["R"]), dev(c["eps"]), outputs=ac.outputs(c), **kw)
    out = dict(x=torch.full_like(got["x"], 7.0))
    again = eng.anticipated_paths(dev(c["B"]), dev(c["C"]), dev(c["T"]), dev(c["R"]), dev(c["eps"]), outputs=("x",), out=out, **kw)
    torch.cuda.synchronize()
    assert again["x"] is out["x"]
    assert_array_equal(again["x"].cpu().numpy(), results(name)["x"])
    for key in ac.outputs(c) + ("status",):
        assert_array_equal(got[key].cpu().numpy(), results(name)[key])


def test_news_without_a_lead_equals_simulate(results):
    c, got = ac.case("sw17_news0"), results("sw17_news0")
    sim = batched.simulate_batched(c["T"], c["R"], np.ascontiguousarray(c["E"][:, :, :, 0]), x0=c["X0"])["paths"]
    err = np.abs(got["x"] - sim).max() / np.abs(sim).max()
    print(f"news with n_lead = 0 against simulate: {err:.2e} of max|x|")
    assert err <= BAR
