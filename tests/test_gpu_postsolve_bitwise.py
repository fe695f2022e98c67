"""The post-solve entries return what their parent commit returned, bit for bit.

tests/golden/postsolve_bitwise_parent.npz was recorded with tools/make_postsolve_bitwise_golden.py from the build of the commit
BEFORE the kernels of these entries were moved onto the shared pieces of csrc/dsge_postsolve.hpp; the cases and what each is there
for are listed in that recipe.  The parity tests hold these kernels to numpy references at 1e-9 .. 1e-12, which a reordered sum
passes; it cannot pass here.  Every array -- outputs stored in full, SHA-256 of the larger ones, statuses, the per-draw NaN flags --
is compared with np.array_equal on its bytes, so that NaN equals NaN and -0.0 does not equal 0.0.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_postsolve_bitwise_golden",
                                                  os.path.join(ROOT, "tools", "make_postsolve_bitwise_golden.py"))
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


def test_fixture_holds_a_failed_draw_through_every_entry(golden):
    """Draw 1 came in failed: it is NaN throughout in every floating-point output of every case, and no other draw is (the
    smoothers' shocks are NaN at period 0 by definition, not throughout)."""
    flags = [k for k in golden.files if k.endswith("_nan_draws")]
    assert {k.split("/")[0] for k in flags} == set(RECIPE.CASES)
    want = np.arange(RECIPE.NB) == RECIPE.FAILED
    for k in flags:
        assert np.array_equal(golden[k], want), k


@pytest.mark.parametrize("case", RECIPE.CASES)
def test_bit_identical_to_parent(golden, case):
    got = RECIPE.run_case(case)
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    # the generated inputs first: a difference there is the generator's, not the kernel's
    assert np.array_equal(got["input_sha256"], want["input_sha256"]), "the inputs of this case are not the recorded ones"
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if not np.array_equal(got[key].reshape(-1).view(np.uint8), want[key].reshape(-1).view(np.uint8)):
            a, b = got[key].reshape(-1), want[key].reshape(-1)
            diff = np.flatnonzero(~((a == b) | ((a != a) & (b != b))))  # (empty: a sign of zero or a NaN payload alone)
            first = f", first at flat index {diff[0]}: {a[diff[0]]!r} != {b[diff[0]]!r}" if len(diff) else ""
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ in value{first}")
