"""GPU: the conditional forecast (dsge_conditional_forecast_batched; csrc/dsge_condfc.hpp) against the numpy reference of
tests/conditional_forecast_reference.py (explicit W from matrix powers, np.linalg.solve; held to three independent formulations
at 1e-10 by tests/test_conditional_forecast_reference.py).

Bar: the project's 1e-9, per output block and draw, on error / max|x| of the draw's reference paths -- no floor at 1: the states
here are about 0.05.  Every accuracy case has cond_2(G) <= 1e5 by the reference alone, and prints its largest error."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched

from tests import conditional_forecast_cases as cc
from tests import smoother_cases

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _run(c, **over):
    return batched.conditional_forecast_batched(c["T"], c["R"], c["Q"], c["x0"], c["conditions"], c["n_steps"], **{**cc.kwargs(c), **over})


@pytest.fixture(scope="module")
def results():
    """The device result of every case, computed on first use and shared (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(cc.case(name))
        return cache[name]

    return get


def _scale(r):
    return np.abs(r["x"]).max(axis=(1, 2, 3))


# ---- parity: m = 8, 16, 17, 40, 49, 64, 96; selector and dense Z; the Q layouts; d; free sets; the condition patterns; p = 1, 16;
# ---- 1, 16, 17 paths; shared / per-draw / per-path x0, eps and values; eps NULL; n_shock_steps < n_steps (the table of CASES) ------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_parity_with_the_reference(results, name):
    c, r, got = cc.case(name), cc.reference(name), results(name)
    assert (r["cond"] <= cc.COND_BAR).all(), r["cond"]
    assert (got["status"] == 0).all()
    scale = _scale(r)
    errs = {}
    for key in ("x", "shocks", "observed"):
        assert got[key].shape == r[key].shape, key
        errs[key] = max(np.abs(got[key][b] - r[key][b]).max() / scale[b] for b in range(cc.NB))
    print(f"{name} (m = {c['m']}, n_cond = {len(c['cond_t'])}, cond(G) <= {r['cond'].max():.1e}):", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_the_conditions_are_met_and_the_shocks_generate_the_path(results, name):
    c, r, got = cc.case(name), cc.reference(name), results(name)
    scale = _scale(r)[:, None, None]
    d = 0.0 if c["d"] is None else c["d"]
    obs = np.einsum("oi,bsti->bsto", c["Z"], got["x"]) + d
    miss = np.abs(obs[:, :, c["cond_t"], c["cond_j"]] - c["V"]) / scale
    sim = batched.simulate_batched(c["T"], c["R"], got["shocks"], x0=c["X0"])["paths"]
    gap = np.abs(sim - got["x"]) / scale[..., None]
    print(f"{name}: conditions missed by {miss.max():.2e}, simulate(shocks_out) differs from x_out by {gap.max():.2e} of max|x|")
    assert miss.max() <= BAR and gap.max() <= BAR
    if c["free"] is not None:  # the shocks that are not free: the baseline, bit for bit (zero where there is none)
        fixed = [j for j in range(c["k"]) if j not in c["free"]]
        base = np.zeros_like(got["shocks"])
        if c["E"] is not None:
            base[:, :, :c["E"].shape[2]] = c["E"]
        assert_array_equal(got["shocks"][..., fixed], base[..., fixed])
    n_eff = max(int(c["cond_t"].max()) + 1, 0 if c["E"] is None else c["E"].shape[2])
    assert (got["shocks"][:, :, n_eff:] == 0).all()  # zero-filled past the last shock that can be non-zero


def test_no_condition_equals_simulate():
    c = cc.case("sw17_subset")
    none = np.full((1, c["p"]), np.nan)
    got = batched.conditional_forecast_batched(c["T"], c["R"], c["Q"], c["x0"], none, c["n_steps"], **cc.kwargs(c))
    sim = batched.simulate_batched(c["T"], c["R"], c["eps"], n_steps=c["n_steps"], x0=c["X0"])["paths"]
    err = np.abs(got["x"] - sim).max() / np.abs(sim).max()
    print(f"n_cond = 0 against simulate: {err:.2e} of max|x|")
    assert err <= BAR and (got["status"] == 0).all()
    assert_array_equal(got["shocks"], c["E"])
    assert np.abs(got["observed"] - (got["x"] @ c["Z"].T + c["d"])).max() <= BAR * np.abs(sim).max()


@pytest.mark.parametrize("name", ["sw17_gap", "sw40_last"])
def test_two_calls_give_the_same_bits(results, name):
    again = _run(cc.case(name))
    for key in ("x", "shocks", "observed", "status"):
        assert_array_equal(again[key], results(name)[key])


# ---- failures ------------------------------------------------------------------------------------------------------------------------
def _singular_inputs():
    """sw40 (shock j moves variable j at impact), series 2 and 4 conditioned, shocks {1, 3, 5} free: with the selector Z nothing
    free reaches the conditioned series (cond(G) ~ 1e30)."""
    c = cc.case("sw40_last")
    rng = np.random.default_rng(5)
    conds = np.full((4, 7), np.nan)
    conds[:, [2, 4]] = 0.02 * rng.standard_normal((4, 2))
    return c, conds, dict(Z=np.eye(7, 40), d=None, eps=c["eps"], n_paths=c["n_paths"], free_shocks=[1, 3, 5], q_mode=c["q_mode"])


def test_unreachable_conditions_set_the_status_bit_and_give_nan():
    c, conds, kw = _singular_inputs()
    got = batched.conditional_forecast_batched(c["T"], c["R"], c["Q"], c["x0"], conds, c["n_steps"], **kw)
    assert (got["status"] == _lib.ST_COND_SINGULAR).all() and _lib.ST_COND_SINGULAR == 512
    assert all(np.isnan(got[key]).all() for key in ("x", "shocks", "observed"))


def test_a_singular_draw_does_not_touch_its_neighbours():
    """Draw 1 keeps the selector Z (singular); in draws 0 and 2 the conditioned series 2 and 4 read variables 1 and 3, which the free
    shocks 1 and 3 move.  The healthy draws must come out with the bits of a call that holds them alone."""
    c, conds, kw = _singular_inputs()
    Z = np.stack([np.eye(7, 40)] * 3)
    for b in (0, 2):
        Z[b, 2], Z[b, 4] = np.eye(40)[1], np.eye(40)[3]
    kw["Z"] = Z
    got = batched.conditional_forecast_batched(c["T"], c["R"], c["Q"], c["x0"], conds, c["n_steps"], **kw)
    assert got["status"].tolist() == [0, 512, 0]
    keep = [0, 2]
    kw.update(Z=Z[keep], eps=c["eps"][keep])
    alone = batched.conditional_forecast_batched(c["T"][keep], c["R"][keep], c["Q"][keep], c["x0"][keep], conds, c["n_steps"], **kw)
    assert (alone["status"] == 0).all()
    for key in ("x", "shocks", "observed"):
        assert np.isnan(got[key][1]).all() and np.isfinite(got[key][keep]).all()
        assert_array_equal(got[key][keep], alone[key])
    # and they are right: the reference of draw 0, path 0
    from tests import conditional_forecast_reference as ref
    ct, cj = np.nonzero(~np.isnan(conds))
    r = ref.conditional_forecast(c["T"][0], c["R"][0], c["Qf"][0], Z[0], None, c["X0"][0, 0], ct, cj, conds[ct, cj], c["n_steps"],
                                 eps=c["E"][0, 0], free=[1, 3, 5])
    assert np.linalg.cond(r["G"]) <= cc.COND_BAR
    assert np.abs(got["x"][0, 0] - r["x"]).max() <= BAR * np.abs(r["x"]).max()


def test_a_failed_draw_between_two_healthy_ones(results):
    c = cc.case("sw17_gap")
    status = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32)
    got = _run(c, status=status)
    assert got["status"].tolist() == [0, _lib.ST_NOT_CONVERGED, 0] and status.tolist() == [0, 1, 0]
    for key in ("x", "shocks", "observed"):
        assert np.isnan(got[key][1]).all()
        assert_array_equal(got[key][[0, 2]], results("sw17_gap")[key][[0, 2]])


@pytest.mark.parametrize("name", ["sw17_subset", "sw40_last"])
def test_device_tensors_equal_the_host_twin(results, name):
    import torch
    from geconpy_amd.engine import LogpEngine

    c, eng = cc.case(name), LogpEngine(0)
    dev = lambda a: None if a is None else eng.to_device(a)  # noqa: E731
    kw = cc.kwargs(c)
    kw.update(Z=dev(c["Z"]), d=dev(c["d"]), eps=dev(c["eps"]))
    got = eng.conditional_forecast(dev(c["T"]), dev(c["R"]), dev(c["Q"]), dev(c["x0"]), dev(c["conditions"]), c["n_steps"], **kw)
    vals = c["conditions"][..., c["cond_t"], c["cond_j"]]
    triple = eng.conditional_forecast(dev(c["T"]), dev(c["R"]), dev(c["Q"]), dev(c["x0"]), (c["cond_t"], c["cond_j"], dev(vals)),
                                      c["n_steps"], **kw)
    torch.cuda.synchronize()
    for key in ("x", "shocks", "observed", "status"):
        assert_array_equal(got[key].cpu().numpy(), results(name)[key])
        assert_array_equal(triple[key].cpu().numpy(), results(name)[key])


def test_the_chain_from_the_filter():
    """kalman_filter_outputs_batched -> the last filtered state as x0 -> the conditional forecast, on sw17_qfull."""
    from tests import conditional_forecast_reference as ref

    s = smoother_cases.case("sw17_qfull")
    f = batched.kalman_filter_outputs_batched(s["T"], s["R"], s["q"], s["Z"], s["y"], Hdiag=s["H"], q_mode=s["q_mode"])
    assert (f["status"] == 0).all()
    x0 = np.ascontiguousarray(f["filtered_states"][:, -1])
    conds = np.full((8, 4), np.nan)
    conds[:, 0] = 0.01 * np.arange(8)  # a path for the first observable, held for eight periods
    got = batched.conditional_forecast_batched(s["T"], s["R"], s["q"], x0, conds, 12, Z=s["Z"], q_mode=s["q_mode"], status=f["status"])
    assert (got["status"] == 0).all()
    ct, cj = np.nonzero(~np.isnan(conds))
    for b in range(s["T"].shape[0]):
        r = ref.conditional_forecast(s["T"][b], s["R"][b], smoother_cases.q_full(s, b), s["Z"], None, x0[b], ct, cj, conds[ct, cj], 12)
        assert np.linalg.cond(r["G"]) <= cc.COND_BAR
        errs = {key: np.abs(got[key][b, 0] - r[key]).max() / np.abs(r["x"]).max() for key in ("x", "shocks", "observed")}
        print(f"chain draw {b}:", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAR
        assert np.abs(got["observed"][b, 0, :8, 0] - conds[:, 0]).max() <= BAR * np.abs(r["x"]).max()
