"""The full step of the tile-layout Kalman filter returns what its parent commit returned, bit for bit, at the smallest shapes that
reach every path of it.

tests/golden/kalman_mf_fullstep_parent.npz was recorded from the build of the commit BEFORE the full step of kalman_mf_kernel
(csrc/dsge_kalman_mf.hpp) lost instructions around its arithmetic, with tools/make_kalman_mf_fullstep_golden.py; the cases and what
each is there for are listed in that recipe: 9, 12, 13, 16, 17, 18 and 20 state variables at p = 1, 7 and 8 (every tile width, the
per-pivot branches, the seven unconditional pivots and the eighth), observed non-states below and above lane 16 and up to 28 retained
variables, a missing-data mask that changes at every step, holds and changes again (a period with no observation and one with a single
observed entry among them), the loop entered, left and entered again, the steady test switched off, a covariance whose diagonal turns
non-finite in one draw, and the record instance through the gradient entry.  `logp`, `status`, `steady_at` and the gradient's
cotangents are compared with np.array_equal (the non-finite draw's logp with equal_nan).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_kalman_mf_fullstep_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_fullstep_golden.py"))
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


def _case(golden, case):
    return {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(ALL)
    assert os.path.getsize(RECIPE.GOLDEN) < 128 << 10  # (kalman_mf_bitwise_parent.npz: 0.3 MB)
    shapes = {(c[0], c[2]) for c in RECIPE.CASES.values()}
    assert {(s, p) for s in (9, 12, 13, 16, 17, 18, 20) for p in (1, 7, 8)} <= shapes
    assert max(c[0] + c[1] for c in RECIPE.CASES.values()) == 28
    # observed non-states whose positions lie below and above lane 16
    assert any(c[1] > 0 and c[0] + c[1] <= 16 for c in RECIPE.CASES.values())
    assert any(c[1] > 0 and c[0] >= 16 for c in RECIPE.CASES.values())
    assert {"complete", "changing"} == {c[3] for c in RECIPE.CASES.values()}
    assert RECIPE.T_LEN <= 64 and RECIPE.NB <= 4


def test_changing_masks_change_hold_and_change_again():
    """The pattern the kept observation weights are rebuilt and reused under."""
    for name, c in RECIPE.CASES.items():
        if c[3] != "changing":
            continue
        mk = RECIPE.case_masks(name)
        full = (1 << c[2]) - 1
        assert all(mk[t] != mk[t + 1] for t in range(RECIPE.HOLD_FROM - 1)), name          # changes at every step
        assert (mk[RECIPE.HOLD_FROM:RECIPE.LEAVE] == full).all(), name                      # holds
        assert mk[RECIPE.LEAVE] != full and mk[RECIPE.LEAVE] == mk[RECIPE.LEAVE + 2], name  # changes again, holds three periods
        assert mk[RECIPE.LEAVE + 3] == 0 and mk[RECIPE.LEAVE + 4] == 1, name                # no observation; a single entry
        assert (mk[RECIPE.LEAVE + 5:] == full).all(), name


@pytest.mark.parametrize("case", ALL)
def test_full_and_steady_steps_run(golden, results, case):
    """A case that runs no full step (or, where it is about the loop, no steady step) checks nothing: at least MIN_FULL full steps
    and MIN_STEADY steady steps in one stretch per draw, in the fixture and now."""
    for at in (golden[f"{case}/steady_at"], results[case]["steady_at"]):
        full, stretch = RECIPE.step_counts(RECIPE.case_masks(case), at)
        assert (full >= RECIPE.MIN_FULL).all(), (at.tolist(), full.tolist())
        if case in RECIPE.LOOP_CASES:
            assert (stretch >= RECIPE.MIN_STEADY).all(), (at.tolist(), stretch.tolist())
    RECIPE.check_case(case, _case(golden, case))


@pytest.mark.parametrize("case", ALL)
def test_bit_identical_to_parent(golden, results, case):
    got, want = results[case], _case(golden, case)
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernel's
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    RECIPE.check_case(case, got)
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        nan_ok = case == "nonfinite_diag" and key == "logp"  # (status and every other array: exactly)
        if not np.array_equal(got[key], want[key], equal_nan=nan_ok):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")
