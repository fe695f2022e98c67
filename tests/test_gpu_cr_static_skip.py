"""The fused likelihood call returns what its parent commit returned, bit for bit, although the one-launch deflated cycle
reduction no longer forms the static rows of T and R where the filter behind it reads none of them (dsge_cr_fused.hpp,
phase 3; docs/design/cycle_reduction.md 4.1i).

tests/golden/cr_static_skip_parent.npz was recorded with tools/make_cr_static_skip_golden.py from the build of the commit
BEFORE that change; the recipe lists the cases and what each is there for.  logp and status of every case are compared with
np.array_equal.  That alone could hold vacuously, so test_static_rows_are_zero_where_the_rule_fires looks at T and R under
dsge_debug_cr_static_rows(2), which applies the rule although the caller receives them: zeros in the static rows of exactly
the draws the recipe expects (expected_skip: told the observation model, taken by a one-launch instance, no deflated variable
observed), every other entry equal to mode 1 (never skip).  Below 17 variables there is no one-launch instance: base_n8,
base_n12, obs_static_n12 and handed_on_n12 run the three launches, which always form the static rows -- they pin "unchanged",
and base_n20 / handed_on_n20 are the smallest shapes on which the rule fires.
The tests without the gpu mark check on the CPU that the generated inputs have the structure the cases claim.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recipe():
    spec = importlib.util.spec_from_file_location("make_cr_static_skip_golden",
                                                  os.path.join(ROOT, "tools", "make_cr_static_skip_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()
LOGP_RTOL = 1e-9  # tests/test_gpu_parity.py: the general filter against the oracle
VISIBLE = ("base_n12", "base_n20", "base_n40", "obs_static_n12", "obs_static_n40", "mixed_n40", "more_static_n40")
FIRES = {  # draws on which the rule fires, as the recipe's docstring describes the cases (None: every draw)
    "base_n8": (), "base_n12": (), "base_n20": None, "base_n37": None, "base_n40": None, "base_n48": None,
    "obs_static_n12": (), "obs_static_n40": (), "mixed_n40": RECIPE.MIXED_STATE_DRAWS, "zbatched_n40": (0, 2, 4),
    "p8_n40": None, "p1_n40": None, "p9_n40": (), "more_static_n40": (0, 2, 3), "rst_singular_n40": None, "nonconv_n40": None,
    "handed_on_n12": (), "handed_on_n20": None,
}


@pytest.fixture(scope="module")
def golden():
    return np.load(RECIPE.GOLDEN)


@pytest.fixture()
def static_rows_mode():
    from geconpy_amd import _lib

    lib = _lib.load()

    def set_mode(mode):
        _lib.check(lib.dsge_debug_cr_static_rows(mode))

    try:
        yield set_mode
    finally:
        _lib.check(lib.dsge_debug_cr_static_rows(0))


@pytest.mark.parametrize("case", RECIPE.CASES)
def test_inputs_have_the_structure_the_cases_claim(case):
    n, ns, nl, k, hint, nb, p, T_len = RECIPE.SHAPES[case]
    a = RECIPE.inputs(case)
    assert 4 <= nb <= 8 and T_len <= 16 and a["A"].shape == (nb, n, n) and a["y"].shape == (T_len, p)
    st, ob = RECIPE.static_mask(case), RECIPE.observed_mask(case)
    h_true = n - ns - nl
    want_static = np.full(nb, h_true)
    if case == "mixed_n40":
        want_static[list(RECIPE.MIXED_STATE_DRAWS)] -= 1
    assert st.sum(axis=1).tolist() == want_static.tolist()
    assert (st.sum(axis=1) >= hint).all()  # no draw is handed over for too few static variables
    assert hint == (h_true - 2 if case == "more_static_n40" else h_true - 1 if case == "mixed_n40" else h_true)
    fires = FIRES[case]
    want = np.ones(nb, dtype=bool) if fires is None else np.isin(np.arange(nb), fires)
    assert RECIPE.expected_skip(case).tolist() == want.tolist()
    if case.startswith("obs_static"):
        assert (ob & st).sum(axis=1).tolist() == [1] * nb
    if case == "mixed_n40":  # variable 18 is observed everywhere; a state in the marked draws, static in the others
        assert ob[:, ns].all() and (st[:, ns] == ~want).all()
    if case == "more_static_n40":  # 26 is static, not deflated and observed in draw 0; 20 is deflated and observed in draw 1
        assert st[0, 26] and ob[0, 26] and st[1, 20] and ob[1, 20] and not (ob & st)[2:].any()
    if case == "zbatched_n40":
        assert a["Z"].shape == (nb, p, n) and (ob & st).sum(axis=1).tolist() == [0, 1] * (nb // 2)
    if case == "rst_singular_n40":
        assert not a["B"][2, :, 21].any() and st[2, 21] and a["B"][[0, 1, 3]][:, :, 21].any(axis=1).all()
    if case.startswith("handed_on"):  # dense, no selector, nothing on the static variables
        assert (a["Z"][:, ~st[0]] != 0).all() and not a["Z"][:, st[0]].any()
    if case == "mixed_n40":  # the replaced draws are solvable systems
        for i in RECIPE.MIXED_STATE_DRAWS:
            assert bool(oracle.cycle_reduction_core(a["A"][i], a["B"][i], a["C"][i], RECIPE.MAX_ITER, RECIPE.TOL)[1]), i


def test_fixture_covers_every_case(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(RECIPE.CASES)
    assert os.path.getsize(RECIPE.GOLDEN) < 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("case", RECIPE.CASES)
def test_logp_and_status_bit_identical_to_parent(golden, case):
    assert np.array_equal(RECIPE.input_sha(case), golden[f"{case}/input_sha256"]), "the inputs of this case are not the recorded ones"
    got = RECIPE.evaluate(case)
    for key in RECIPE.KEYS:
        want = golden[f"{case}/{key}"]
        print(case, key, got[key].tolist())
        assert got[key].dtype == want.dtype and got[key].shape == want.shape, key
        assert np.array_equal(got[key], want, equal_nan=True), (case, key, got[key].tolist(), want.tolist())
    if case in ("rst_singular_n40", "nonconv_n40"):  # the draws meant to fail do fail, as at the parent
        bad = [2] if case == "rst_singular_n40" else list(range(len(got["status"])))
        assert (got["status"][bad] != 0).all() and (np.delete(got["status"], bad) == 0).all(), got["status"]
    else:
        assert (got["status"] == 0).all(), got["status"]


def _policy(case, set_mode, mode):
    n, _, _, k, _, nb, _, _ = RECIPE.SHAPES[case]
    set_mode(mode)
    out = dict(T=np.full((nb, n, n), np.nan), R=np.full((nb, n, k), np.nan))
    return RECIPE.evaluate(case, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("case", VISIBLE)
def test_static_rows_are_zero_where_the_rule_fires(static_rows_mode, case):
    hint = RECIPE.SHAPES[case][4]
    full = _policy(case, static_rows_mode, 1)
    skip = _policy(case, static_rows_mode, 2)
    default = _policy(case, static_rows_mode, 0)  # the caller receives T and R: every row
    fires, st = RECIPE.expected_skip(case), RECIPE.static_mask(case)
    assert np.array_equal(skip["status"], full["status"]) and (full["status"] == 0).all()
    for key in ("T", "R", "logp", "status"):
        assert np.array_equal(default[key], full[key]), key
    for i in range(len(fires)):
        rows = np.flatnonzero(st[i])[:hint]  # the deflated variables
        others = np.setdiff1d(np.arange(st.shape[1]), rows)
        for key in ("T", "R"):
            assert np.isfinite(skip[key][i]).all()
            assert np.array_equal(skip[key][i][others], full[key][i][others]), (case, i, key)
            if fires[i]:
                assert not skip[key][i][rows].any() and not np.signbit(skip[key][i][rows]).any(), (case, i, key)
                assert full[key][i][rows].any(), (case, i, key)  # (what was skipped is not zero by itself)
            else:
                assert np.array_equal(skip[key][i][rows], full[key][i][rows]), (case, i, key)
    # logp of a draw is the same number whichever way its static rows were left
    assert np.array_equal(skip["logp"], full["logp"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("handed_on_n12", "handed_on_n20"))
def test_general_filter_on_zeroed_static_rows(static_rows_mode, case):
    a = RECIPE.inputs(case)
    static_rows_mode(0)
    got = RECIPE.evaluate(case)
    static_rows_mode(1)
    full = RECIPE.evaluate(case)
    assert (got["status"] == 0).all(), got["status"]
    rel = np.abs(got["logp"] - full["logp"]) / np.abs(full["logp"])
    print(case, "largest relative difference of logp to mode 1:", rel.max())
    for i in range(len(got["logp"])):
        ref = oracle.solve_kalman_logp(a["A"][i], a["B"][i], a["C"][i], a["D"][i], np.diag(a["sig"][i] ** 2), a["Z"], a["y"],
                                       H=np.diag(a["Hdiag"]), tol=RECIPE.TOL, max_iter=RECIPE.MAX_ITER)
        np.testing.assert_allclose(got["logp"][i], ref["logp"], rtol=LOGP_RTOL)
