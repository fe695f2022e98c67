"""The cycle-reduction kernels return what their parent commit returned, bit for bit.

tests/golden/cr_bitwise_parent.npz was recorded from the build of the commit BEFORE the instruction cuts in the blocked
elimination (gauss_jordan_blocked, csrc/dsge_device.hpp) with tools/make_cr_bitwise_golden.py; the cases and what each is
there for are listed in that recipe.  The other bit-identity tests of the suite compare kernels that share the elimination
with each other (compact against dense, fused against three launches, ...), so a change that moves all of them together
passes there; it cannot pass here.  Every array is compared with np.array_equal: T, R (or the selection output of the entry
used), status, iteration counts, logp, and the cotangents of the gradient entry.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_cr_bitwise_golden", os.path.join(ROOT, "tools", "make_cr_bitwise_golden.py"))
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


@pytest.mark.parametrize("case", RECIPE.CASES)
def test_bit_identical_to_parent(golden, case):
    got = RECIPE.run_case(case)
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernels'
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    assert (got["status"] == 0).all(), got["status"]
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if not np.array_equal(got[key], want[key]):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")
