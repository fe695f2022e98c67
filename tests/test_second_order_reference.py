"""The oracle of the second-order path (oracle/second_order.py) on the problems of tests/second_order_cases.py, before the device is held
to it (tests/test_gpu_second_order_edges.py).  No GPU.  The device bars there (1e-9 of a coefficient block's largest entry, 1e-8
relative on logp) are justified here from the reference's side:

  (a) for n <= 24 the reduced formulation (Schur form on the state block) and the full one (Kronecker system on all n^2 columns) agree
      to 1e-12 of each block's largest entry: the floor of the reference (from n = 20 on draw 0 only: the full system has n^3 unknowns,
      7 s per draw at n = 20 and 11 s at n = 24);
  (b) CONDITIONING: moving every entry of A, B, C, D by 1e-11 of its size moves every coefficient block by at most 1e-10 of its largest
      entry and logp by at most 1e-10 relative, so a device solve good to 1e-13 leaves nine tenths of either bar to the kernels;
  (c) logp with the four blocks zeroed differs from logp by at least 1e-6 relative (100 x the logp bar): the case sees the second-order
      terms;
  (d) |logp| >= 0.1 sum_t |ll_t|: no near-cancelling sum under the relative bar on logp;
  (e) m and u are the table's and the tile instance is the one the case is named for.

Besides, the shapes beyond the entry's limits are refused by its argument check, before any device work.

A case that fails is given another seed in second_order_cases.SEEDS, never a wider bar."""
import numpy as np
import pytest

import oracle
from oracle import second_order as so

from tests import second_order_cases as sc

FLOOR = 1e-12
CONDITION_REL, CONDITION_BAR = 1e-11, 1e-10
VISIBLE = 1e-6
CANCELLATION = 0.1
FULL_MAX_N, FULL_BOTH_DRAWS_MAX_N = 24, 16
PROBLEMS = sc.CASES + tuple(sc.NESTED)
# the variants that share the system of their base share its coefficients: (a) runs once per system
SYSTEMS = tuple(sc.SHAPES)


def _scale(x):
    return max(np.abs(x).max(), 1e-300)


@pytest.mark.parametrize("name", PROBLEMS)
def test_dimensions_and_tile_instance(name):
    if name in sc.NESTED:
        base, _, m, mt = sc.NESTED[name]
        u = sc.SHAPES[base][0][5] + sc.NESTED[name][1]
    else:
        (_, _, _, _, _, u), m, mt = sc.SHAPES[name.split("_", 1)[0] if name not in sc.SHAPES else name]
    pr = sc.problem(name)
    for r in sc.reference(name):
        assert (r["m"], r["u"]) == (m, u), (name, r["m"], r["u"])
        assert sc.so_tiles(r["m"]) == mt, (name, r["m"])
    assert pr["y"].shape[1] == pr["Z"].shape[0]
    assert [sc.so_tiles(m_) for m_ in (32, 33, 64, 65, 112, 113, 160, 161, 208, 209)] == [2, 4, 4, 7, 7, 10, 10, 13, 13, 0]


@pytest.mark.parametrize("name", [s_ for s_ in SYSTEMS if sc.SHAPES[s_][0][0] <= FULL_MAX_N])
def test_the_two_formulations_agree(name):
    pr = sc.problem(name)
    n, k = pr["D"].shape[1:]
    worst = dict.fromkeys(sc.BLOCKS, 0.0)
    for i, r in enumerate(sc.reference(name)[:2 if n <= FULL_BOTH_DRAWS_MAX_N else 1]):
        a = sc.draw(pr, i)
        sol = r["sol"]
        S = np.asarray(sol["S"])
        full = so.second_order_solution(a["A"], a["B"], a["C"], a["D"], so.hessian_coo_to_dense(n, k, pr["idx"], pr["val"][i]), r["T"], r["R"],
                                        a["Sigma"])
        gyy = full["g_yy"].reshape(n, n, n)
        gyu = full["g_yu"].reshape(n, n, k)
        off = np.setdiff1d(np.arange(n), S)
        # (outside the state columns the full solution vanishes: the policy depends on y- through S only)
        assert np.abs(gyy[:, off, :]).max(initial=0.0) <= FLOOR * _scale(gyy) and np.abs(gyy[:, :, off]).max(initial=0.0) <= FLOOR * _scale(gyy)
        assert np.abs(gyu[:, off, :]).max(initial=0.0) <= FLOOR * _scale(gyu)
        pairs = {"g_yy": gyy[:, S][:, :, S], "g_yu": gyu[:, S], "g_uu": full["g_uu"].reshape(n, k, k), "g_ss": full["g_ss"]}
        for key in sc.BLOCKS:
            worst[key] = max(worst[key], np.abs(pairs[key] - sol[key]).max() / _scale(sol[key]))
    print(name, " ".join(f"{k_} {v:.1e}" for k_, v in worst.items()))
    assert max(worst.values()) <= FLOOR, worst


@pytest.mark.parametrize("name", PROBLEMS)
def test_conditioning_of_every_draw(name):
    pr = sc.problem(name)
    rng = np.random.default_rng([5, *name.encode()])
    worst = {}
    for i, r in enumerate(sc.reference(name)):
        moved = so.solve_second_order_logp(**sc.draw(pr, i, perturb=(rng, CONDITION_REL)))
        for key in sc.BLOCKS:
            worst[key, i] = np.abs(moved["sol"][key] - r["sol"][key]).max() / _scale(r["sol"][key])
        worst["logp", i] = abs(moved["logp"] - r["logp"]) / abs(r["logp"])
    print(name, " ".join(f"{k_}[{i}] {v:.1e}" for (k_, i), v in worst.items()))
    assert max(worst.values()) <= CONDITION_BAR, worst


@pytest.mark.parametrize("name", PROBLEMS)
def test_second_order_terms_are_visible_and_logp_does_not_cancel(name):
    pr = sc.problem(name)
    for i, r in enumerate(sc.reference(name)):
        a = sc.draw(pr, i)
        zero = {key: np.zeros_like(r["sol"][key]) for key in sc.BLOCKS}
        flat = so.pruned_kalman_logp(r["T"], r["R"], dict(zero, S=r["sol"]["S"]), a["Sigma"], a["Z"], a["y"], H=a["H"], d=a["d"])
        lp, ps, P0 = so.pruned_kalman_logp(r["T"], r["R"], r["sol"], a["Sigma"], a["Z"], a["y"], H=a["H"], d=a["d"], return_parts=True)
        assert lp == r["logp"]
        total, ll = oracle.kalman_filter_logp(a["y"], ps["Az"], np.eye(ps["m"]), ps["Qz"], so.pruned_design(a["Z"], a["d"], ps["U"], ps["m"]),
                                              H=a["H"], d=a["d"], c=ps["c"], a0=ps["mean"], P0=P0, return_per_step=True)
        assert total == lp
        print(name, i, f"logp {lp:.6g} sum|ll_t| {np.abs(ll).sum():.6g} second-order terms {abs(flat - lp) / abs(lp):.1e}")
        assert abs(flat - lp) >= VISIBLE * abs(lp), (name, i, flat, lp)
        assert abs(lp) >= CANCELLATION * np.abs(ll).sum(), (name, i, lp, np.abs(ll).sum())


def test_out_of_range_shapes_are_refused_before_the_device_is_touched():
    """m = 210, u = 41, k = 13, p = 9 and k > s: DSGE_ERR_INVALID from the entry's own argument check, which runs before the device is
    initialised and before the first-order solver can write status_out (no GPU is needed to see the refusal; the device-side half --
    the caller's buffers keep their bits -- is tests/test_gpu_second_order_edges.py::test_refusals_leave_the_outputs_alone)."""
    from geconpy_amd import _lib, batched

    for name, (pr, limit) in sc.refused().items():
        args, kwargs = sc.entry_point_arguments(pr)
        with pytest.raises(_lib.DsgeHipError) as refusal:
            batched.second_order_logp_batched(*args, **kwargs, return_solution=True)
        assert refusal.value.code == _lib.ERR_INVALID, (name, refusal.value)
        assert "second order" in str(refusal.value) and limit in str(refusal.value), (name, limit, refusal.value)
    # ... and so is a retained list that does not begin with the states (it used to be refused after the first-order solve)
    pr = sc.problem("k_eq_s")
    args, kwargs = sc.entry_point_arguments(pr)
    S, Lc, U = batched.second_order_structure(pr["A"], pr["C"], pr["Z"])
    with pytest.raises(_lib.DsgeHipError) as refusal:
        batched.second_order_logp_batched(*args, **kwargs, structure=(S, Lc, U[::-1].copy()))
    assert refusal.value.code == _lib.ERR_INVALID and "states first" in str(refusal.value), refusal.value
