"""GPU: perfect-foresight paths under an occasionally binding bound (dsge_constrained_paths_batched; csrc/dsge_obc.hpp) against the
numpy reference of tests/constrained_reference.py (np.linalg.solve on Mz[S,S], the regime iteration as defined; held to the
regime-switched stacked-time system and to brute force over all binding sets at 1e-10 by tests/test_constrained_reference.py).

Bars: x, w and observed at 1e-9 of the draw's reference max|x| per output block, no floor at 1 (the bar of
tests/test_gpu_anticipated.py); nu at 1e-9 of max|nu|, gap at 1e-9 of max|q|, Mz at 1e-9 of max|Mz|; iters and path_status equal
the reference's entry by entry.  Every accuracy case meets, by the reference alone, the conditions of
tests/test_constrained_reference.py::check_conditions, and prints its largest errors."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched

from tests import constrained_cases as cc
from tests.test_constrained_reference import check_conditions

pytestmark = pytest.mark.gpu

BAR = 1e-9
PATH_KEYS = ("x", "w", "observed", "nu", "gap")


def _run(c, **over):
    kw = {**cc.kwargs(c), "outputs": cc.outputs(c), **over}
    return batched.constrained_paths_batched(*cc.args(c), **kw)


@pytest.fixture(scope="module")
def results():
    """The device result of every case, computed on first use and shared (never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(cc.case(name))
        return cache[name]

    return get


def _errors(c, r, got):
    """Largest error of every output block in units of its scale, over draws (and paths, for nu and gap)."""
    errs = {}
    scale = np.abs(r["x"]).max(axis=(1, 2, 3))
    for key in ("x", "w") + (("observed",) if c["p"] else ()):
        assert got[key].shape == r[key].shape, key
        errs[key] = max(np.abs(got[key][b] - r[key][b]).max() / scale[b] for b in range(cc.NB))
    nu_scale = np.abs(r["nu"]).max()
    errs["nu"] = np.abs(got["nu"] - r["nu"]).max() / nu_scale if nu_scale > 0.0 else float(np.abs(got["nu"]).max())
    errs["gap"] = (np.abs(got["gap"] - r["gap"]).max(axis=-1) / r["qmax"]).max()
    errs["Mz"] = max(np.abs(got["Mz"][b] - r["Mz"][b]).max() / np.abs(r["Mz"][b]).max() for b in range(cc.NB))
    return errs


# ---- parity: the table of cc.CASES ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_parity_with_the_reference(results, name):
    c, r, got = cc.case(name), cc.reference(name), results(name)
    f = check_conditions(name)
    assert (got["status"] == 0).all()
    assert_array_equal(got["iters"], r["iters"])
    assert_array_equal(got["path_status"], r["path_status"])
    errs = _errors(c, r, got)
    print(f"{name} (n = {c['n']}, H = {c['horizon']}, {c['n_paths']} paths, iters <= {f['iters']}, margin {f['margin']:.1e}, "
          f"cond(Mz[S,S]) <= {f['cond_S']:.1e}):", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR, errs


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_complementarity_holds_on_the_device_output(results, name):
    c, r, got = cc.case(name), cc.reference(name), results(name)
    H = c["horizon"]
    assert (got["nu"] >= 0.0).all()
    assert (got["gap"][:, :, :H] >= -BAR * r["qmax"][:, :, None]).all()
    slack = np.abs(got["nu"] * got["gap"][:, :, :H]).sum(axis=-1)
    assert (slack <= BAR * np.abs(got["nu"]).max(axis=-1) * r["qmax"]).all()


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_the_anticipated_paths_on_the_shadow_shocks_give_the_same_bits(results, name):
    c, got = cc.case(name), results(name)
    H, s = c["horizon"], c["shock"]
    e = np.zeros((cc.NB, c["n_paths"], max(c["n_shock"], H), c["k"]))
    e[:, :, :c["n_shock"]] = c["E"]
    e[:, :, :H, s] += got["nu"]
    outs = ("x", "w") + (("observed",) if c["p"] else ())
    again = batched.anticipated_paths_batched(c["B"], c["C"], c["T"], c["R"], e, **cc.kwargs(c), outputs=outs)
    for key in outs:
        assert_array_equal(again[key], got[key])


def test_without_a_binding_period_the_bits_are_those_of_the_anticipated_paths(results):
    c, got = cc.case("rbc_none"), results("rbc_none")
    assert (got["nu"] == 0.0).all() and (got["iters"] == 1).all()
    plain = batched.anticipated_paths_batched(c["B"], c["C"], c["T"], c["R"], c["eps"], **cc.kwargs(c), outputs=("x", "w"))
    for key in ("x", "w"):
        assert_array_equal(plain[key], got[key])


@pytest.mark.parametrize("name", ["nk_iters", "sw40_h33"])
def test_two_calls_give_the_same_bits(results, name):
    again = _run(cc.case(name))
    for key in cc.outputs(cc.case(name)) + ("status",):
        assert_array_equal(again[key], results(name)[key])


@pytest.mark.parametrize("name", ["rbc_beyond", "nk_iters", "sw64_h64"])
def test_any_subset_of_the_outputs_gives_the_same_bits(results, name):
    """x alone holds the paths itself, without it they live in library scratch; nu, Mz or iters alone skip the final paths."""
    c = cc.case(name)
    every = cc.outputs(c)
    for outs in tuple((key,) for key in every) + (("x", "gap"), ("w", "nu", "path_status")):
        got = _run(c, outputs=outs)
        assert sorted(got) == sorted(outs + ("status",))
        for key in outs + ("status",):
            assert_array_equal(got[key], results(name)[key])


def test_draws_beyond_one_chunk_of_unit_paths_give_the_same_bits(results):
    """The unit paths that give Mz run in chunks of draws whose parked terms fit 256 MB (launch_obc.hip): 128 draws at n = H = 64.
    The three draws of sw64_h64 repeated 44 times make 132 draws, two chunks of 66, and every copy -- in either chunk, across
    their boundary -- must carry the bits of the small call."""
    c, small = cc.case("sw64_h64"), results("sw64_h64")
    reps = 44
    assert c["n"] == c["horizon"] == 64 and cc.NB * reps > (256 << 20) // (64 * 64 * 64 * 8)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))  # noqa: E731
    kw = dict(cc.kwargs(c), x0=tile(c["x0"]))
    got = batched.constrained_paths_batched(*(tile(c[key]) for key in ("B", "C", "T", "R", "eps", "Cr", "Bd")), c["shock"], c["horizon"],
                                            **kw, outputs=cc.outputs(c))
    assert (got["status"] == 0).all()
    for key in cc.outputs(c):
        for i in (0, 21, 22, reps - 1):
            assert_array_equal(got[key][cc.NB * i:cc.NB * (i + 1)], small[key])


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nk_iters", "sw17_h17", "sw40_h32"])
def test_device_tensors_equal_the_host_twin(results, name):
    import torch
    from geconpy_amd.engine import LogpEngine

    c, eng = cc.case(name), LogpEngine(0)
    dev = lambda a: eng.to_device(a) if isinstance(a, np.ndarray) else a  # noqa: E731
    kw = {key: dev(v) for key, v in cc.kwargs(c).items()}
    args = [dev(a) for a in cc.args(c)]
    got = eng.constrained_paths(*args, outputs=cc.outputs(c), **kw)
    out = dict(x=torch.full_like(got["x"], 7.0), nu=torch.full_like(got["nu"], 7.0))
    again = eng.constrained_paths(*args, outputs=("x", "nu"), out=out, **kw)
    torch.cuda.synchronize()
    assert again["x"] is out["x"] and again["nu"] is out["nu"]
    for key in ("x", "nu"):
        assert_array_equal(again[key].cpu().numpy(), results(name)[key])
    for key in cc.outputs(c) + ("status",):
        assert_array_equal(got[key].cpu().numpy(), results(name)[key])


# ---- failures stay local ---------------------------------------------------------------------------------------------------------------
def _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, full, failed):
    """``failed`` (NB, n_paths) bool: those paths are NaN in every path output, every other path has the bits of ``full``."""
    for key in (k for k in PATH_KEYS if k in got):
        assert np.isnan(got[key][failed]).all(), key
        assert_array_equal(got[key][~failed], full[key][~failed])
        assert np.isfinite(got[key][~failed]).all(), key


def test_too_few_iterations_leave_exactly_the_reference_s_paths_without_a_regime(results):
    c, full = cc.case("nk_iters"), results("nk_iters")
    r2 = cc.reference("nk_iters", 2)
    failed = r2["path_status"] == _lib.OBC_NO_REGIME
    assert failed.any() and not failed.all() and (cc.reference("nk_iters")["iters"][failed] > 2).all()
    got = _run(c, max_iter=2)
    assert_array_equal(got["path_status"], r2["path_status"])
    assert_array_equal(got["iters"], r2["iters"])
    assert got["status"].tolist() == [_lib.ST_CONSTRAINT_UNRESOLVED if row.any() else 0 for row in failed]
    assert _lib.ST_CONSTRAINT_UNRESOLVED == 4096
    _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, full, failed)
    assert_array_equal(got["Mz"], full["Mz"])


def test_a_zero_constraint_row_makes_its_draw_s_paths_singular_and_no_other(results):
    """c = 0 with a bound above zero on draw 1: Mz = 0 and q = -bound < 0 in every period."""
    c, full = cc.case("sw40_h33"), results("sw40_h33")
    Cr, Bd = c["Cr"].copy(), c["Bd"].copy()
    Cr[1], Bd[1] = 0.0, 0.5
    got = batched.constrained_paths_batched(c["B"], c["C"], c["T"], c["R"], c["eps"], Cr, Bd, c["shock"], c["horizon"], **cc.kwargs(c),
                                            outputs=cc.outputs(c))
    failed = np.zeros((cc.NB, c["n_paths"]), bool)
    failed[1] = True
    assert (got["path_status"][1] == _lib.OBC_SINGULAR).all() and (got["iters"][1] == 1).all()
    assert_array_equal(got["path_status"][[0, 2]], full["path_status"][[0, 2]])
    assert got["status"].tolist() == [0, _lib.ST_CONSTRAINT_UNRESOLVED, 0]
    assert (got["Mz"][1] == 0.0).all()
    _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, full, failed)


@pytest.mark.parametrize("how", ["singular", "status"])
def test_a_skipped_draw_does_not_touch_its_neighbours(results, how):
    """A draw whose M = B + C T has a zero row (the construction of tests/test_gpu_anticipated.py, rank_tol = 1e-10 at n = 64), or
    that comes in with a status word: SKIPPED and NaN, the status word as the anticipated-shock entry leaves it."""
    c, full = cc.case("sw64_h64"), results("sw64_h64")
    B, status, kw = c["B"], None, {}
    if how == "singular":
        B = c["B"].copy()
        B[1, 2] = -(c["C"][1] @ c["T"][1])[2]
        kw, want = dict(rank_tol=1e-10), [0, _lib.ST_ANTICIPATION_SINGULAR, 0]
    else:
        status, want = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32), [0, _lib.ST_NOT_CONVERGED, 0]
    got = batched.constrained_paths_batched(B, *cc.args(c)[1:], **cc.kwargs(c), outputs=cc.outputs(c), status=status, **kw)
    failed = np.zeros((cc.NB, c["n_paths"]), bool)
    failed[1] = True
    assert got["status"].tolist() == want
    assert (got["path_status"][1] == _lib.OBC_SKIPPED).all() and (got["iters"][1] == 0).all() and np.isnan(got["Mz"][1]).all()
    assert_array_equal(got["path_status"][[0, 2]], full["path_status"][[0, 2]])
    assert_array_equal(got["iters"][[0, 2]], full["iters"][[0, 2]])
    assert_array_equal(got["Mz"][[0, 2]], full["Mz"][[0, 2]])
    if how == "status":  # (rank_tol = 1e-10 is another threshold for the healthy draws' pivots too, not other bits)
        _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, full, failed)
    else:
        again = batched.constrained_paths_batched(*cc.args(c), **cc.kwargs(c), outputs=cc.outputs(c), **kw)
        _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, again, failed)
        _assert_failed_paths_are_nan_and_the_rest_untouched(c, got, full, failed)


def test_a_violation_beyond_the_horizon_is_reported_and_the_path_returned(results):
    c, r, got = cc.case("rbc_beyond"), cc.reference("rbc_beyond"), results("rbc_beyond")
    assert (r["path_status"] & _lib.OBC_BEYOND_HORIZON).any() and _lib.OBC_BEYOND_HORIZON == 4
    assert_array_equal(got["path_status"], r["path_status"])
    assert (got["status"] == 0).all()
    for key in ("x", "w", "nu", "gap"):
        assert np.isfinite(got[key]).all()
    assert max(_errors(c, r, got).values()) <= BAR
