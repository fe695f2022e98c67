"""The refinement branch of the cycle reduction replays the recorded elimination: same bits as eliminating a second time.

crc_iterate (csrc/dsge_cr_compact.hpp) refines the solve of an iteration whose pivots span more than the tile's ratio.  The
correction A1^-1 (R - A1 X) used to come from a second blocked elimination of [A1 | R - A1 X]; it now comes from gj_replay on the
multipliers the first elimination left in the dead panel columns of W -- in the instances with the register budget of two waves
per SIMD (cr_compact_kernel_occ2, cr_fused_kernel_occ2); the others eliminate twice as before and are pinned all the same.
tests/golden/cr_refine_replay_parent.npz holds what the build BEFORE that change returned on the cases of
tools/make_cr_refine_replay_golden.py (the recipe lists them and what each is there for); every output is compared bit for bit
(np.array_equal on the words).  That a case refines at all -- it could pass by not refining -- is
asserted on the host: the numpy replay of the iteration and of the pivots (host_pivot_ratios) puts every system built to refine
a factor ten or more beyond its tile's rule.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_cr_refine_replay_golden as recipe  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(recipe.GOLDEN) as z:
        return {key: z[key] for key in z.files}


def test_the_fixture_holds_every_case(golden):
    assert {key.split("/")[0] for key in golden} == set(recipe.CASES)
    for name in recipe.CASES:
        assert np.array_equal(golden[f"{name}/input_sha256"], recipe.input_sha(name)), name


@pytest.mark.parametrize("name", recipe.CASES)
def test_every_case_refines_on_the_host(name):
    a = recipe.inputs(name)
    nb, n = a["A"].shape[:2]
    assert nb <= 16
    if name == "late_n30":  # the first system refines late (in two iterations), the others never
        rule = recipe.refine_rule(n)
        ratios = [recipe.host_pivot_ratios(a["A"][i], a["B"][i], a["C"][i]) for i in range(nb)]
        assert ratios[0][0] < rule / 10 and (ratios[0][1:] > 10 * rule).sum() >= 2, ratios[0]
        assert all(r.max() < rule / 10 for r in ratios[1:]), ratios[1:]
        return
    if name in ("late_n40", "late_fused_n40"):
        if name == "late_fused_n40":  # what the one-launch kernel iterates on: the reduced system, on the 4-wide tile
            hint = recipe.FUSED[name][4]
            red = [recipe.reduced_system(a["A"][i], a["B"][i], a["C"][i], hint) for i in range(nb)]
            rule = recipe.refine_rule(n - hint)
            ratios = [recipe.host_pivot_ratios(*r, tol=1e-8) for r in red]
        else:
            rule = recipe.refine_rule(n)
            ratios = [recipe.host_pivot_ratios(a["A"][i], a["B"][i], a["C"][i]) for i in range(nb)]
        for i in recipe.LATE_REFINING:  # late: not in the first iteration, then a factor ten beyond the rule
            assert ratios[i][0] < rule / 10 and ratios[i][1:].max() > 10 * rule, (i, ratios[i])
        assert (ratios[0] > 10 * rule).sum() >= 2  # ... and in more than one iteration
        assert (ratios[2] > 10 * rule).all()  # draw 752: in every iteration, the first included
        assert all(r.max() < rule / 10 for r in ratios[3:])  # plain draws next to them
        return
    for i in range(nb):
        if not a["refines"][i]:
            continue
        if name in recipe.FUSED:
            hint = recipe.FUSED[name][4]
            A, B, C = recipe.reduced_system(a["A"][i], a["B"][i], a["C"][i], hint)
        else:
            A, B, C = a["A"][i], a["B"][i], a["C"][i]
        ratios = recipe.host_pivot_ratios(A, B, C)
        assert ratios[0] > 10 * recipe.refine_rule(A.shape[0]), (name, i, ratios)
        if not name.startswith("three_launch"):
            assert (ratios > 10 * recipe.refine_rule(A.shape[0])).sum() >= 2, (name, i, ratios)  # more than one iteration


@pytest.mark.parametrize("name", recipe.CASES)
def test_bit_identical_to_the_parent(golden, name):
    got = recipe.evaluate(name)
    for key in recipe.keys(name):
        want = golden[f"{name}/{key}"]
        g = np.ascontiguousarray(got[key])
        assert g.shape == want.shape and g.dtype == want.dtype, (name, key, g.shape, g.dtype, want.shape, want.dtype)
        if g.dtype == np.float64:  # the bits: a NaN of another sign or payload is a difference
            g, want = g.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
        assert np.array_equal(g, want), (name, key, np.argwhere(g != want)[:8].tolist())
    a = recipe.inputs(name)
    if a["refines"] is not None and name != "mixed_n30":
        assert not got["status"].any(), got["status"].tolist()


def test_mixed_batch_has_every_kind(golden):
    """mixed_n30: refining, plain, not converging, NaN, refining -- the failing draws fail, the others do not notice."""
    st = golden["mixed_n30/status"]
    assert st[0] == 0 and st[1] == 0 and st[4] == 0 and st[2] != 0 and st[3] != 0, st.tolist()
