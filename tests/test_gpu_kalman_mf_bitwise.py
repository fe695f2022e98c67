"""The tile-layout Kalman filter returns what its parent commit returned, bit for bit.

tests/golden/kalman_mf_bitwise_parent.npz was recorded from the build of the commit BEFORE the instruction cuts in kalman_mf_kernel
(csrc/dsge_kalman_mf.hpp) with tools/make_kalman_mf_bitwise_golden.py; the cases and what each is there for are listed in that
recipe.  The parity tests compare the kernel with the VALU filter kernels to 1e-11, which a reordered sum passes; it cannot pass
here.  Every array is compared with np.array_equal: logp, status, the first steady step, the per-step outputs, the cotangents.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_kalman_mf_bitwise_golden",
                                                  os.path.join(ROOT, "tools", "make_kalman_mf_bitwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()


@pytest.fixture(scope="module")
def golden():
    return np.load(RECIPE.GOLDEN)


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(RECIPE.CASES)
    assert os.path.getsize(RECIPE.GOLDEN) < 1 << 20


def test_fixture_runs_both_modes(golden):
    """The recorded steady steps say which code the cases ran: the steady loop on draws 0..3, 200 full steps on draw 3437 and under
    kalman_steady_tol = 0, a switch in every instance shape."""
    assert (golden["sw_fused/steady_at"] > 0).all() and (golden["sw_fused/steady_at"] < 100).all()
    assert golden["sw_never_steady/steady_at"][0] == -1
    assert (golden["sw_full_recursion/steady_at"] == -1).all()
    for name in RECIPE.STANDALONE:
        assert (golden[f"{name}/steady_at"] > 0).all(), name
    # scattered missing data: the mask changes before the covariance settles, no draw ever switches; a block of missing periods
    # AFTER the switch: the switch is where it is without the block (the steady mode is then left and resumed)
    assert (golden["sw_nan10/steady_at"] == -1).all()
    assert np.array_equal(golden["sw_missing_block/steady_at"], golden["sw_fused/steady_at"])
    assert (golden["sw_missing_block/steady_at"] < 90).all()
    # observed jump variables: every draw switches, the never-steady draw of the plain model included
    assert (golden["sw_jumps/steady_at"] > 0).all()


def test_jump_case_runs_the_tile_kernel(golden):
    """sw_jumps is there for the seven-group second pass (kalman_mf_kernel<5,7>: 18 state variables + 7 observed jump variables = 25
    retained, more than the <5,5> instance holds).  Its outputs cannot say which kernel wrote them, so: the VALU cascade
    (kalman_mfma = 0), which is where a routing change would send these draws, sums in another order and must NOT reproduce the
    fixture bit for bit -- if it does, the fixture pins the wrong kernel."""
    valu = RECIPE.run_case("sw_jumps", extra_options={"kalman_mfma": 0})
    assert (valu["status"] == 0).all(), valu["status"]
    np.testing.assert_allclose(valu["logp"], golden["sw_jumps/logp"], rtol=1e-9)
    assert not np.array_equal(valu["logp"], golden["sw_jumps/logp"])


@pytest.mark.parametrize("case", RECIPE.CASES)
def test_bit_identical_to_parent(golden, case):
    got = RECIPE.run_case(case)
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernel's
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    assert (got["status"] == 0).all(), got["status"]
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if not np.array_equal(got[key], want[key]):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")
