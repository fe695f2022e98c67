"""GPU: the stochastic simulation at an occasionally binding bound (dsge_constrained_simulate_batched; csrc/dsge_obc_sim.hpp) against
the numpy reference of tests/constrained_sim_reference.py (written by the definition, not through the kernels' tables; held to
period 0 of the perfect-foresight reference, to the table form and to time consistency at 1e-10 by
tests/test_constrained_sim_reference.py).

Bars, those of tests/test_gpu_constrained.py: x and observed at 1e-9 of the draw's reference max|x|, no floor at 1; gap at 1e-9 of
the path's largest max|q| over periods; shadow and plan at 1e-9 of max|plan|; Mz at 1e-9 of max|Mz|; iters, duration, path_status
and fail_step equal the reference's entry by entry.  Every accuracy case meets, by the reference alone, the conditions of
tests/test_constrained_sim_reference.py::check_conditions, and prints its largest errors."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched

from tests import constrained_sim_cases as sc
from tests.test_constrained_sim_reference import check_conditions

pytestmark = pytest.mark.gpu

BAR = 1e-9
STEP_KEYS = ("x", "observed", "gap", "shadow", "plan")


def _run(c, **over):
    kw = {**sc.kwargs(c), "outputs": sc.outputs(c), **over}
    return batched.constrained_simulate_batched(*sc.args(c), **kw)


@pytest.fixture(scope="module")
def results():
    """The device result of every case, computed on first use and shared (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(sc.case(name))
        return cache[name]

    return get


def _errors(c, r, got):
    """Largest error of every output block in units of its scale."""
    errs = {}
    scale = np.abs(r["x"]).max(axis=(1, 2, 3))
    for key in ("x",) + (("observed",) if c["p"] else ()):
        assert got[key].shape == r[key].shape, key
        errs[key] = max(np.abs(got[key][b] - r[key][b]).max() / scale[b] for b in range(sc.NB))
    errs["gap"] = (np.abs(got["gap"] - r["gap"]).max(axis=-1) / r["qmax"].max(axis=-1)).max()
    plan_scale = np.abs(r["plan"]).max()
    for key in ("shadow", "plan"):
        err = np.abs(got[key] - r[key]).max()
        errs[key] = err / plan_scale if plan_scale > 0.0 else float(err)
    errs["Mz"] = max(np.abs(got["Mz"][b] - r["Mz"][b]).max() / np.abs(r["Mz"][b]).max() for b in range(sc.NB))
    return errs


# ---- parity: the accuracy cases of sc.CASES ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ACCURACY)
def test_parity_with_the_reference(results, name):
    c, r, got = sc.case(name), sc.reference(name), results(name)
    f = check_conditions(name)
    assert (got["status"] == 0).all()
    for key in ("iters", "duration", "path_status", "fail_step"):
        assert got[key].dtype == np.int32
        assert_array_equal(got[key], r[key], err_msg=key)
    errs = _errors(c, r, got)
    print(f"{name} (n = {c['n']}, H = {c['horizon']}, {c['n_paths']} paths, {c['n_steps']} steps, iters <= {f['iters']}, duration <= "
          f"{f['duration']}, margin {f['margin']:.1e}, cond(Mz[S,S]) <= {f['cond_S']:.1e}):",
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("name", sc.ACCURACY)
def test_complementarity_holds_on_the_device_output(results, name):
    c, r, got = sc.case(name), sc.reference(name), results(name)
    qmax = r["qmax"].max(axis=-1)[:, :, None]
    assert (got["plan"] >= 0.0).all() and (got["shadow"] == got["plan"][..., 0]).all()
    assert (got["gap"] >= -BAR * qmax).all()
    assert (np.abs(got["shadow"] * got["gap"]) <= BAR * np.abs(got["plan"]).max() * qmax).all()
    mz = batched.constrained_paths_batched(*sc.args(c), n_steps=c["horizon"], outputs=("Mz",))["Mz"]
    assert_array_equal(got["Mz"], mz)


# ---- against the perfect-foresight entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nk_h17", "sw40_h32", "sw64_h64"])
def test_one_step_is_period_0_of_the_perfect_foresight_entry(name):
    c = sc.case(name)
    H, e0 = c["horizon"], np.ascontiguousarray(c["E"][:, :, :1])
    args = (c["B"], c["C"], c["T"], c["R"], e0, c["c"], c["bound"], c["shock"], H)
    got = batched.constrained_simulate_batched(*args, n_steps=1, x0=c["x0"], outputs=("x", "plan", "iters"))
    pf = batched.constrained_paths_batched(*args, n_steps=H, x0=c["x0"], outputs=("x", "nu", "iters", "path_status"))
    assert (pf["path_status"] & ~_lib.OBC_BEYOND_HORIZON == 0).all() and (pf["nu"] > 0.0).any()
    assert_array_equal(got["iters"][:, :, 0], pf["iters"])
    for b in range(sc.NB):
        assert np.abs(got["x"][b, :, 0] - pf["x"][b, :, 0]).max() <= BAR * np.abs(pf["x"][b]).max()
    assert np.abs(got["plan"][:, :, 0] - pf["nu"]).max() <= BAR * np.abs(pf["nu"]).max()


def test_replanning_every_period_reproduces_the_perfect_foresight_entry_s_path(results):
    name = "sw40_t0"
    c, got = sc.case(name), results(name)
    pf = batched.constrained_paths_batched(*sc.args(c), **sc.kwargs(c), outputs=("x", "path_status", "nu"))
    ok = pf["path_status"] == 0
    assert ok.any() and (pf["nu"][ok] > 0.0).any()
    for b in range(sc.NB):
        assert np.abs(got["x"][b][ok[b]] - pf["x"][b][ok[b]]).max() <= BAR * np.abs(pf["x"][b][ok[b]]).max()


# ---- the same bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nk_h17", "sw40_h33"])
def test_two_calls_give_the_same_bits(results, name):
    again = _run(sc.case(name))
    for key in sc.outputs(sc.case(name)) + ("status",):
        assert_array_equal(again[key], results(name)[key])


@pytest.mark.parametrize("name", ["rbc_h8", "nk_h17", "sw64_h64"])
def test_every_single_output_gives_the_bits_of_the_full_call(results, name):
    c = sc.case(name)
    for key in sc.outputs(c):
        got = _run(c, outputs=(key,))
        assert sorted(got) == sorted((key, "status"))
        assert_array_equal(got[key], results(name)[key])
        assert_array_equal(got["status"], results(name)["status"])


@pytest.mark.parametrize("name", ["nk_h17", "sw17_h17", "sw40_h32"])
def test_device_tensors_equal_the_host_twin(results, name):
    import torch
    from geconpy_amd.engine import LogpEngine

    c, eng = sc.case(name), LogpEngine(0)
    dev = lambda a: eng.to_device(a) if isinstance(a, np.ndarray) else a  # noqa: E731
    kw = {key: dev(v) for key, v in sc.kwargs(c).items()}
    args = [dev(a) for a in sc.args(c)]
    got = eng.constrained_simulate(*args, outputs=sc.outputs(c), **kw)
    out = dict(x=torch.full_like(got["x"], 7.0), plan=torch.full_like(got["plan"], 7.0))
    again = eng.constrained_simulate(*args, outputs=("x", "plan"), out=out, **kw)
    torch.cuda.synchronize()
    assert again["x"] is out["x"] and again["plan"] is out["plan"]
    for key in ("x", "plan"):
        assert_array_equal(again[key].cpu().numpy(), results(name)[key])
    for key in sc.outputs(c) + ("status",):
        assert_array_equal(got[key].cpu().numpy(), results(name)[key])


# ---- failures stay local ---------------------------------------------------------------------------------------------------------------
def _assert_failure_layout(c, got, r, full=None):
    """Where the reference names a failure at period f: NaN from f on, iters the count at f then 0, duration -1; before f -- and on
    every path that did not fail -- the bits of ``full`` (if given)."""
    assert_array_equal(got["path_status"], r["path_status"])
    assert_array_equal(got["fail_step"], r["fail_step"])
    assert_array_equal(got["iters"], r["iters"])
    assert_array_equal(got["duration"], r["duration"])
    steps = np.arange(c["n_steps"])
    dead = (r["fail_step"][:, :, None] >= 0) & (steps >= r["fail_step"][:, :, None])
    for key in (k for k in STEP_KEYS if k in got):
        assert np.isnan(got[key][dead]).all() and np.isfinite(got[key][~dead]).all(), key
        if full is not None:
            assert_array_equal(got[key][~dead], full[key][~dead])


def test_too_few_iterations_fail_exactly_where_the_reference_says(results):
    name = "sw40_h32"
    c, full, r2 = sc.case(name), results(name), sc.reference(name, 2)
    failed = (r2["path_status"] & _lib.OBC_NO_REGIME) != 0
    assert failed.any() and not failed.all() and (r2["fail_step"][failed] > 0).any()
    got = _run(c, max_iter=2)
    _assert_failure_layout(c, got, r2, full)
    assert got["status"].tolist() == [_lib.ST_CONSTRAINT_UNRESOLVED if row.any() else 0 for row in failed]
    assert_array_equal(got["Mz"], full["Mz"])


def test_a_matrix_without_a_regime_fails_where_the_reference_says(results):
    c, r, got = sc.case("nk_fails"), sc.reference("nk_fails"), results("nk_fails")
    failed = (r["path_status"] & _lib.OBC_NO_REGIME) != 0
    assert failed.any() and not failed.all()
    _assert_failure_layout(c, got, r)
    assert got["status"].tolist() == [_lib.ST_CONSTRAINT_UNRESOLVED if row.any() else 0 for row in failed]
    scale = np.abs(np.nan_to_num(r["x"])).max(axis=(1, 2, 3))
    err = max(np.nanmax(np.abs(got["x"][b] - r["x"][b])) / scale[b] for b in range(sc.NB))
    assert err <= BAR


def test_a_zero_constraint_row_makes_its_draw_s_paths_singular_and_no_other(results):
    """c = 0 with a bound above zero on draw 1: Mz = 0 and q = -bound < 0 in every period, from period 0 on."""
    name = "sw40_h33"
    c, full = sc.case(name), results(name)
    Cr, Bd = c["Cr"].copy(), c["Bd"].copy()
    Cr[1], Bd[1] = 0.0, 0.5
    got = batched.constrained_simulate_batched(c["B"], c["C"], c["T"], c["R"], c["eps"], Cr, Bd, c["shock"], c["horizon"], **sc.kwargs(c),
                                               outputs=sc.outputs(c))
    assert (got["path_status"][1] == _lib.OBC_SINGULAR).all() and (got["fail_step"][1] == 0).all()
    assert (got["iters"][1, :, 0] == 1).all() and (got["iters"][1, :, 1:] == 0).all() and (got["duration"][1] == -1).all()
    assert got["status"].tolist() == [0, _lib.ST_CONSTRAINT_UNRESOLVED, 0]
    assert (got["Mz"][1] == 0.0).all()
    for key in sc.outputs(c):
        assert_array_equal(got[key][[0, 2]], full[key][[0, 2]])
    for key in (k for k in STEP_KEYS if k in got):
        assert np.isnan(got[key][1]).all(), key


@pytest.mark.parametrize("how", ["singular", "status"])
def test_a_skipped_draw_does_not_touch_its_neighbours(results, how):
    """A draw whose M = B + C T has a zero row (the construction of tests/test_gpu_anticipated.py, rank_tol = 1e-10 at n = 64), or
    that comes in with a status word: SKIPPED, NaN everywhere, fail_step 0, the status word as the anticipated-shock entry leaves it."""
    name = "sw64_h64"
    c, full = sc.case(name), results(name)
    B, status, kw = c["B"], None, {}
    if how == "singular":
        B = c["B"].copy()
        B[1, 2] = -(c["C"][1] @ c["T"][1])[2]
        kw, want = dict(rank_tol=1e-10), [0, _lib.ST_ANTICIPATION_SINGULAR, 0]
    else:
        status, want = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32), [0, _lib.ST_NOT_CONVERGED, 0]
    got = batched.constrained_simulate_batched(B, *sc.args(c)[1:], **sc.kwargs(c), outputs=sc.outputs(c), status=status, **kw)
    assert got["status"].tolist() == want
    assert (got["path_status"][1] == _lib.OBC_SKIPPED).all() and (got["fail_step"][1] == 0).all()
    assert (got["iters"][1] == 0).all() and (got["duration"][1] == -1).all() and np.isnan(got["Mz"][1]).all()
    for key in (k for k in STEP_KEYS if k in got):
        assert np.isnan(got[key][1]).all(), key
    # (rank_tol = 1e-10 is another threshold for the healthy draws' pivots too, not other bits)
    for key in sc.outputs(c):
        assert_array_equal(got[key][[0, 2]], full[key][[0, 2]])


# ---- grid edges ---------------------------------------------------------------------------------------------------------------------------
def test_draws_beyond_one_chunk_of_unit_paths_give_the_same_bits(results):
    """The unit paths that give Mz run in chunks of draws whose parked terms fit 256 MB (launch_obc.hip): 128 draws at n = H = 64.
    The three draws of sw64_h64 repeated 44 times make 132 draws, two chunks of 66, and every copy must carry the bits of the
    small call (the construction of tests/test_gpu_constrained.py)."""
    c, small = sc.case("sw64_h64"), results("sw64_h64")
    reps = 44
    assert c["n"] == c["horizon"] == 64 and sc.NB * reps > (256 << 20) // (64 * 64 * 64 * 8)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))  # noqa: E731
    kw = dict(sc.kwargs(c), x0=tile(c["x0"]))
    got = batched.constrained_simulate_batched(*(tile(c[key]) for key in ("B", "C", "T", "R", "eps", "Cr", "Bd")), c["shock"],
                                               c["horizon"], **kw, outputs=sc.outputs(c))
    assert (got["status"] == 0).all()
    for key in sc.outputs(c):
        for i in (0, 21, 22, reps - 1):
            assert_array_equal(got[key][sc.NB * i:sc.NB * (i + 1)], small[key])
