"""The fused deflated launch and the three launches return what their parent commit returned, bit for bit, on the branches
of the code outside the iterations: the static mask and the column loads, the reflector passes, the deposit into the LDS tile
and the parked right-hand sides, the gather of the solution and the back-substitution of the static rows.

tests/golden/cr_fused_outside_parent.npz was recorded with tools/make_cr_fused_outside_golden.py from the build of the commit
BEFORE the instruction cuts in those phases; the recipe lists the cases and what each is there for.  Every array -- T, R,
status, iteration counts, logp -- is compared with np.array_equal, for the fused launch and for cr_deflate -> cr_compact ->
cr_inflate.  test_inputs_converge_on_the_oracle needs no GPU: every system converges on the CPU oracle, the handed-over draws
included, so that no comparison here is one of two failures.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_cr_fused_outside_golden",
                                                  os.path.join(ROOT, "tools", "make_cr_fused_outside_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()


@pytest.fixture(scope="module")
def golden():
    return np.load(RECIPE.GOLDEN)


@pytest.mark.parametrize("case", RECIPE.CASES)
def test_inputs_converge_on_the_oracle(case):
    A, B, C, _, _, hint = RECIPE.inputs(case)
    n = A.shape[-1]
    static = ~((A != 0).any(axis=1) | (C != 0).any(axis=1))  # (draw, variable)
    for i in range(RECIPE.NB):
        _, converged, _ = oracle.cycle_reduction_core(A[i], B[i], C[i], RECIPE.MAX_ITER, RECIPE.TOL)
        assert bool(converged), (case, i)
        assert (static[i].sum() < hint) == (case == "fewer_static" and i == 3), (case, i, int(static[i].sum()), n)
    if case == "more_static":
        assert (static.sum(axis=1) > hint).all()
    if case == "static_rows":  # the planted columns: non-zero, and only in the rows of the static variables
        st = static[0]
        assert (A[:4, :, n - 2][:, st] != 0).all() and not A[:4, :, n - 2][:, ~st].any()
        assert (C[4:, :, 2][:, st] != 0).all() and not C[4:, :, 2][:, ~st].any()


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(RECIPE.CASES)
    assert os.path.getsize(RECIPE.GOLDEN) < 1 << 20


def _compare(case, got, want):
    assert (got["status"] == 0).all(), got["status"]
    for key in RECIPE.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if not np.array_equal(got[key], want[key]):
            diff = np.argwhere(got[key] != want[key])
            pytest.fail(f"{case}/{key}: {len(diff)} of {want[key].size} entries differ, first at {diff[0].tolist()}: "
                        f"{got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", (1, 0), ids=("fused", "three_launches"))
@pytest.mark.parametrize("case", RECIPE.CASES)
def test_bit_identical_to_parent(golden, case, fused):
    # the generated inputs first: a difference there is the generator's, not the kernels'
    assert np.array_equal(RECIPE._sha(*RECIPE.inputs(case)[:5]), golden[f"{case}/input_sha256"]), \
        "the inputs of this case are not the recorded ones"
    prefix = case + "/" if fused or bool(golden[f"{case}/3l/same"]) else case + "/3l/"
    _compare(case, RECIPE.run_case(case, fused), {key: golden[prefix + key] for key in RECIPE.KEYS})
