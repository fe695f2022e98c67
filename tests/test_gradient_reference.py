"""The autograd reference of the gradient (tests/gradient_reference.py) on the problems of tests/gradient_cases.py, before the
device is held to it (tests/test_gpu_gradient_entries.py).  No GPU.

  * its logp is the oracle's (1e-12 relative);
  * its two formulations -- implicit Newton step + Kronecker Lyapunov solve, unrolled cycle reduction + doubling series -- agree on
    every entry of every block to 1e-12 of the block's scale (measured: 4e-14 at worst): the floor of the reference;
  * three entries per block (largest, median, smallest non-zero) agree with Richardson-extrapolated central differences of the
    oracle, entry by entry;
  * CONDITIONING, a condition on the inputs: a relative perturbation of 1e-11 of A, B, C, D moves the gradient by at most 1e-8 of
    each block's scale (amplification <= 1e3), so that a device solve good to 1e-13 leaves nine tenths of the 1e-9 bar to the
    kernels.  A draw that fails is replaced by another seed in gradient_cases.py, never excused."""
import functools

import numpy as np
import pytest

import oracle

from tests import gradient_cases as gc
from tests import gradient_reference as gr

FLOOR = 1e-12
CONDITION_REL, CONDITION_BAR = 1e-11, 1e-8
# the oracle's logp carries rounding noise of a few 1e-13 relative (test_gradient_rbc_against_extrapolated_differences: ~1e-13); the
# extrapolation (16 (4 D(h/4) - D(h/2)) / 3 - (4 D(h/2) - D(h)) / 3) / 15 of central differences D multiplies a noise delta per
# evaluation by ~4.6 / h, so with delta <= 4e-13 max(1, |logp|):
FD_NOISE = 2e-12
FD_GATE, FD_RTOL = 1e-5, 1e-7  # (test_gradient_sw_shaped_against_extrapolated_differences: converged to 1e-5 -> compared at 1e-7)
FD_STEPS = (2e-3, 5e-4, 8e-3)  # relative to the size of the input entry; the first that has converged is used


@functools.lru_cache(maxsize=None)
def _unrolled(name):
    pr = gc.problem(name)
    return {i: gr.logp_and_gradient(formulation="unrolled", **gc.draw(pr, i)) for i in pr["draws"]}


def _scale(x):
    return max(np.abs(x).max(), 1e-300)


def test_every_case_has_a_problem_with_a_reference():
    for name, c in gc.CASES.items():
        pr = gc.problem(c["problem"])
        assert c["problem"] in gc.PROBLEMS and len(pr["draws"]) >= 2, name
        assert pr["y"].ndim == 2 and pr["y"].shape[1] == pr["Z"].shape[-2], name


@pytest.mark.parametrize("name", gc.PROBLEMS)
def test_logp_is_the_oracles(name):
    pr = gc.problem(name)
    for i, ref in gc.reference(name).items():
        a = gc.draw(pr, i)
        Q = a["Q"] if "Q" in a else np.diag(a["q"])
        want = oracle.solve_kalman_logp(a["A"], a["B"], a["C"], a["D"], Q, a["Z"], a["y"], H=np.diag(a["Hdiag"]), d=a["d"], tol=1e-15,
                                        max_iter=300, conventions=a["conventions"])["logp"]
        assert abs(ref["logp"] - want) <= 1e-12 * abs(want), (i, ref["logp"], want)
        assert abs(_unrolled(name)[i]["logp"] - want) <= 1e-12 * abs(want), (i, _unrolled(name)[i]["logp"], want)


@pytest.mark.parametrize("name", gc.PROBLEMS)
def test_the_two_formulations_agree_on_every_entry(name):
    pr = gc.problem(name)
    worst = {}
    for i, ref in gc.reference(name).items():
        other = _unrolled(name)[i]
        assert set(gc.blocks(pr)) <= set(ref) and set(ref) == set(other)
        for key in gc.blocks(pr):
            assert ref[key].shape == other[key].shape and np.isfinite(ref[key]).all()
            worst[key] = max(worst.get(key, 0.0), np.abs(ref[key] - other[key]).max() / _scale(ref[key]))
    print(name, " ".join(f"{k_} {v:.1e}" for k_, v in worst.items()))
    assert max(worst.values()) <= FLOOR, worst


@pytest.mark.parametrize("name", gc.PROBLEMS)
def test_conditioning_of_every_draw(name):
    pr = gc.problem(name)
    rng = np.random.default_rng([5, *name.encode()])
    worst = {}
    for i in pr["draws"]:
        base = _unrolled(name)[i]
        moved = gr.logp_and_gradient(formulation="unrolled", **gc.draw(pr, i, perturb=(rng, CONDITION_REL)))
        for key in gc.blocks(pr):
            worst[key, i] = np.abs(moved[key] - base[key]).max() / _scale(base[key])
    print(name, " ".join(f"{k_}[{i}] {v:.1e}" for (k_, i), v in worst.items()))
    assert max(worst.values()) <= CONDITION_BAR, worst


def _oracle_logp(a, **moved):
    a = dict(a, **moved)
    Q = a["Q"] if "Q" in a else np.diag(a["q"])
    return oracle.solve_kalman_logp(a["A"], a["B"], a["C"], a["D"], Q, a["Z"], a["y"], H=np.diag(a["Hdiag"]), d=a["d"], tol=1e-15,
                                    max_iter=300, conventions=a["conventions"])["logp"]


def _entries(g, allowed):
    """Indices of the largest, the median and the smallest non-zero entry of |g| among ``allowed``."""
    idx = np.argwhere((g != 0) & allowed)
    order = np.argsort(np.abs(g[tuple(idx.T)]))
    return [tuple(idx[j]) for j in dict.fromkeys((order[-1], order[len(order) // 2], order[0]))]


def _extrapolated(f, h):
    d1 = [(f(h / 2 ** j) - f(-h / 2 ** j)) / (2.0 * h / 2 ** j) for j in range(3)]
    d2 = [(4.0 * d1[j + 1] - d1[j]) / 3.0 for j in range(2)]
    d3 = (16.0 * d2[1] - d2[0]) / 15.0
    return d3, abs(d3 - d2[1])


@pytest.mark.parametrize("name", gc.PROBLEMS)
def test_entries_against_extrapolated_differences_of_the_oracle(name):
    """Entry (r, c) of a block is the derivative of the oracle's logp along that one input entry.  Steps: absolute for A, B, C, D, Z
    (entries of order one) and d (0.01), relative for the variances q, Hdiag; a full Q moves along E_rc + E_cr (the oracle is held
    symmetric), whose derivative is twice the entry off the diagonal."""
    pr = gc.problem(name)
    i = pr["draws"][0]
    ref = gc.reference(name)[i]
    a = gc.draw(pr, i)
    noise = FD_NOISE * max(1.0, abs(ref["logp"]))
    inputs = {"A_bar": "A", "B_bar": "B", "C_bar": "C", "D_bar": "D", "q_bar": "q", "Q_bar": "Q", "d_bar": "d", "h_bar": "Hdiag", "Z_bar": "Z"}
    for key in gc.blocks(pr):
        x = a[inputs[key]]
        allowed = np.ones(x.shape, dtype=bool)
        if key == "A_bar":  # the derivative along an entry of a structurally zero column is not part of the contract
            allowed &= (x != 0).any(axis=0)[None, :]
        for at in _entries(ref[key], allowed):
            size = {"q_bar": abs(x[at]), "h_bar": abs(x[at]), "d_bar": 0.01}.get(key, 1.0)
            factor = 1.0
            if key == "Q_bar":
                size = np.sqrt(x[at[0], at[0]] * x[at[1], at[1]])
                factor = 1.0 if at[0] == at[1] else 2.0

            def f(e):
                moved = x.copy()
                moved[at] += e
                if key == "Q_bar" and at[0] != at[1]:
                    moved[at[::-1]] += e
                return _oracle_logp(a, **{inputs[key]: moved})

            for step in FD_STEPS:
                fd, gap = _extrapolated(f, step * size)
                tol_noise = noise / (step * size)
                if gap <= FD_GATE * abs(fd) + tol_noise:
                    break
            else:
                raise AssertionError(f"{name} {key}{at}: the extrapolation did not converge ({fd}, {gap})")
            got = factor * ref[key][at]
            assert abs(got - fd) <= FD_RTOL * abs(fd) + tol_noise, (name, key, at, got, fd, tol_noise)
