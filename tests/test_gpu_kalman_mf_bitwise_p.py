"""The tile-layout Kalman filter returns what its parent commit returned, bit for bit, at p = 8, 6 and 1.

tests/golden/kalman_mf_bitwise_p_parent.npz was recorded from the build of the commit BEFORE the row broadcasts of the F elimination
and of the steady loop's innovation (csrc/dsge_kalman_mf.hpp) with tools/make_kalman_mf_bitwise_p_golden.py; the cases and what each is
there for are listed in that recipe.  tests/test_gpu_kalman_mf_bitwise.py pins p = 3, 4, 5 and 7; the elimination has a path of its
own for p = 8 (pivot 7 behind a branch), for p = 6 (the last branch of the ladder) and for p = 1 (a single pivot), and at p = 8 the
observation mask changes inside the steady loop.  Every array is compared with np.array_equal.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_kalman_mf_bitwise_p_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_bitwise_p_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()


@pytest.fixture(scope="module")
def golden():
    return np.load(RECIPE.GOLDEN)


@pytest.fixture(scope="module")
def results():
    """Every case once, shared by the tests below."""
    return {name: RECIPE.run_case(name) for name in RECIPE.CASES}


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(RECIPE.CASES)
    assert os.path.getsize(RECIPE.GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", list(RECIPE.CASES))
def test_steady_loop_runs(golden, results, case):
    """Every draw switches to the steady loop, in the fixture and now, and before the missing entries of step 120 and later: the mask
    changes INSIDE the steady loop.  The log-likelihoods are of a size at which one rounding shows (mask_d: see the recipe)."""
    for at in (golden[f"{case}/steady_at"], results[case]["steady_at"]):
        assert (at > 0).all() and (at < 120).all(), at
    assert (np.abs(golden[f"{case}/logp"]) < 1e5).all(), golden[f"{case}/logp"]


@pytest.mark.parametrize("case", list(RECIPE.CASES))
def test_case_runs_the_tile_kernel(golden, case):
    """The outputs cannot say which kernel wrote them, so: the VALU cascade (kalman_mfma = 0), which is where a routing change would
    send these draws, sums in another order and must NOT reproduce the fixture bit for bit -- if it does, the fixture pins the wrong
    kernel."""
    valu = RECIPE.run_case(case, extra_options={"kalman_mfma": 0})
    assert (valu["status"] == 0).all(), valu["status"]
    np.testing.assert_allclose(valu["logp"], golden[f"{case}/logp"], rtol=1e-9)
    np.testing.assert_allclose(valu["logp_full"], golden[f"{case}/logp_full"], rtol=1e-9)
    assert not np.array_equal(valu["logp"], golden[f"{case}/logp"])
    assert not np.array_equal(valu["logp_full"], golden[f"{case}/logp_full"])


@pytest.mark.parametrize("case", list(RECIPE.CASES))
def test_bit_identical_to_parent(golden, results, case):
    got = results[case]
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernel's
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    assert (got["status"] == 0).all() and (got["status_full"] == 0).all(), (got["status"], got["status_full"])
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if not np.array_equal(got[key], want[key]):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")
