"""The steady loop of the tile-layout Kalman filter returns what its parent commit returned, bit for bit, at every width of its mean
prediction.

tests/golden/kalman_mf_steady_parent.npz was recorded from the build of the commit BEFORE the mean prediction of the steady loop
(csrc/dsge_kalman_mf.hpp) took the filtered mean by lane swaps and row broadcasts instead of read-lanes, with
tools/make_kalman_mf_steady_golden.py; the cases and what each is there for are listed in that recipe: 9 to 20 state variables (both
sides of the NS - 2 rule at every tile width), 15, 16, 17 and 28 retained variables (below, at and across the 16-lane row boundary,
the maximum), p = 1, 7 and 8, complete data, a stretch of the loop with no observation, a mask change that leaves the loop and
enters it again, the record instance through the gradient entry, and one draw whose filtered mean is not finite.  Every array is
compared with np.array_equal (the non-finite draw's logp with equal_nan).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_kalman_mf_steady_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_steady_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()
ALL = tuple(RECIPE.CASES) + RECIPE.EXTRA


@pytest.fixture(scope="module")
def golden():
    return np.load(RECIPE.GOLDEN)


@pytest.fixture(scope="module")
def results():
    """Every case once, shared by the tests below."""
    return {name: RECIPE.run_case(name) for name in ALL}


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(ALL)
    assert os.path.getsize(RECIPE.GOLDEN) < 1 << 20
    # both sides of the NS - 2 rule at every tile width; the retained variables and the observation counts asked for
    assert sorted({c[0] for c in RECIPE.CASES.values()}) == list(range(9, 21))
    assert {15, 16, 17, 28} <= {c[0] + c[1] for c in RECIPE.CASES.values()}
    assert {1, 7, 8} == {c[2] for c in RECIPE.CASES.values()}
    assert {"complete", "no_obs", "reenter"} == {c[3] for c in RECIPE.CASES.values()}
    assert RECIPE.T_LEN <= 64 and 4 <= RECIPE.NB <= 8


@pytest.mark.parametrize("case", ALL)
def test_steady_loop_runs(golden, results, case):
    """A case that never enters the loop checks nothing: every draw ran at least MIN_STEADY steady steps in one stretch, in the
    fixture and now."""
    for at in (golden[f"{case}/steady_at"], results[case]["steady_at"]):
        stretch = RECIPE.steady_stretch(case, at)
        assert (stretch >= RECIPE.MIN_STEADY).all(), (at.tolist(), stretch.tolist())
    RECIPE.check_case(case, {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")})


@pytest.mark.parametrize("case", ALL)
def test_bit_identical_to_parent(golden, results, case):
    got = results[case]
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernel's
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    RECIPE.check_case(case, got)
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        nan_ok = case == "nonfinite" and key == "logp"  # (status and every other array: exactly)
        if not np.array_equal(got[key], want[key], equal_nan=nan_ok):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")
