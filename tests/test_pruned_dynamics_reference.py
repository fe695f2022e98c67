"""CPU: the numpy restatement of the second-order dynamics (tests/pruned_dynamics_reference.py) against the oracle's own pruned
simulation, the properties the definition implies, and the refusals of the front end (no library is loaded)."""
import numpy as np
import pytest

from geconpy_amd import _lib, batched
from oracle import second_order as so

from tests import dynamics_reference as dr
from tests import pruned_dynamics_reference as pr

ORACLE_BAR = 1e-13


def _shocks(c, i, n_paths, n_steps, seed):
    return np.random.default_rng(seed).standard_normal((n_paths, n_steps, c["sigma"].shape[1])) * c["sigma"][i]


@pytest.mark.parametrize("name", ["n6", "n17", "n40"])
def test_restatement_matches_the_oracle(name):
    """1e-13 x scale per part, 1, 2 and 40 steps; the oracle takes the reduced solution scattered into its n^2 layout."""
    c = pr.case(name)
    for i in range(2):
        T, R, sol = pr.draw(c, i)
        full = pr.full_layout(sol, T.shape[0])
        for n_steps in (1, 2, 40):
            eps = _shocks(c, i, 1, n_steps, 11 + n_steps)[0]
            ref_f, ref_s = so.simulate_pruned(T, R, full, eps)
            got_f, got_s = pr.simulate_pruned(T, R, sol, eps)
            for got, ref in ((got_f, ref_f[1:]), (got_s, ref_s[1:])):
                err = np.abs(got - ref).max() / np.abs(ref).max()
                print(name, i, n_steps, f"{err:.2e}")
                assert err <= ORACLE_BAR


def test_first_order_part_of_a_girf_is_the_linear_response():
    c = pr.case("n17")
    T, R, sol = pr.draw(c, 0)
    S_imp = np.random.default_rng(3).standard_normal((R.shape[1], 4)) * 0.01
    eps = _shocks(c, 0, 3, 5, 4)
    x0 = (np.random.default_rng(5).normal(0, 0.01, (3, T.shape[0])), np.random.default_rng(6).normal(0, 0.001, (3, T.shape[0])))
    gf, _ = pr.girf_pruned(T, R, sol, 12, S_imp, eps, x0)
    ref = dr.impulse_responses(T, R, 12, S_imp)
    assert np.abs(gf - ref).max() <= 1e-13 * np.abs(ref).max()


def test_zero_second_order_blocks_give_the_linear_model():
    c = pr.case("n6")
    T, R, sol = pr.draw(c, 1)
    zero = {key: np.zeros_like(v) if key != "S" else v for key, v in sol.items()}
    eps = _shocks(c, 1, 2, 6, 8)
    _, xs = pr.simulate_pruned(T, R, zero, eps[0], 9)
    assert not xs.any()
    gf, gs = pr.girf_pruned(T, R, zero, 9, None, eps)
    assert not gs.any()
    ref = dr.impulse_responses(T, R, 9)
    assert np.abs(gf - ref).max() <= 1e-13 * np.abs(ref).max()


def test_without_shocks_the_correction_accumulates_the_constant():
    """x_s[t] = (I + T + ... + T^t) 1/2 g_ss."""
    c = pr.case("n17")
    T, R, sol = pr.draw(c, 2)
    _, xs = pr.simulate_pruned(T, R, sol, None, 20)
    acc, term = np.zeros(T.shape[0]), 0.5 * sol["g_ss"]
    for t in range(20):
        acc = acc + term
        term = T @ term
        assert np.abs(xs[t] - acc).max() <= 1e-13 * np.abs(acc).max()


def test_girf_is_sign_asymmetric_at_second_order():
    """What the feature exists for: the x_s parts of the responses to +S_j and to -S_j are not mirror images -- their sum, zero in a
    linear model, exceeds 1e-6 of the response's scale on the n = 40 case."""
    c = pr.case("n40")
    T, R, sol = pr.draw(c, 0)
    k = R.shape[1]
    S_imp = np.diag(c["sigma"][0])
    eps = _shocks(c, 0, 2, 8, 21)
    pf, ps = pr.girf_pruned(T, R, sol, 20, S_imp, eps)
    mf, ms = pr.girf_pruned(T, R, sol, 20, -S_imp, eps)
    scale = np.abs(pf + ps).max()
    assert np.abs(pf + mf).max() <= 1e-13 * scale  # the first-order parts mirror each other
    asym = np.abs(ps + ms).max() / scale
    print("asymmetry / scale", f"{asym:.2e}")
    assert asym > 1e-6
    assert ps.shape == (k, 20, T.shape[0])


def test_malformed_calls_are_value_errors_before_anything_is_staged(monkeypatch):
    def no_library(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    c = pr.case("n6")
    sol = pr.solution(c)
    nb, n, k = c["R"].shape
    s = len(c["S"])
    eps = np.zeros((2, 3, k))
    good_x0 = (np.zeros((2, n)), np.zeros((2, n)))
    cases = [
        ("eps must be", dict(eps=np.zeros((2, 3, k + 1)))),
        ("less than the 3 shock steps", dict(n_steps=2)),
        ("strictly ascending", dict(S=c["S"][::-1])),
        ("strictly ascending", dict(S=np.array([0, 1, 1]))),
        ("strictly ascending", dict(S=np.array([0, 1, n]))),
        ("strictly ascending", dict(S=np.array([-1, 1, 2]))),
        ("length g_yy.shape", dict(S=np.arange(s + 1))),
        ("one shape", dict(x0=(np.zeros((2, n)), np.zeros((nb, 2, n))))),
        ("x0 must be", dict(x0=(np.zeros((3, n)), np.zeros((3, n))))),
        ("pair", dict(x0=np.zeros((2, n)))),
        ("g_yu must be", dict(g_yu=np.zeros((nb, n, s, k + 1)))),
        ("status must be", dict(status=np.zeros(nb + 1, dtype=np.int32))),
    ]
    for match, change in cases:
        kw = dict(eps=eps, n_steps=None, x0=good_x0, status=None)
        this = dict(sol)
        for key, v in change.items():
            (this if key in sol else kw).__setitem__(key, v)
        with pytest.raises(ValueError, match=match):
            batched.simulate_pruned_batched(this, **kw)
        with pytest.raises(ValueError, match=match):
            batched.simulate_pruned_batched(*(this[key] for key in ("T", "R", "g_yy", "g_yu", "g_uu", "g_ss", "S")), **kw)
        with pytest.raises(ValueError, match=match):
            batched.girf_pruned_batched(this, n_steps=5 if kw["n_steps"] is None else kw["n_steps"], eps=kw["eps"], x0=kw["x0"],
                                        status=kw["status"])
    with pytest.raises(ValueError, match="impulses must be"):
        batched.girf_pruned_batched(sol, impulses=np.zeros((k + 1, 2)))
    with pytest.raises(TypeError, match="lacks"):
        batched.simulate_pruned_batched({key: v for key, v in sol.items() if key != "g_ss"}, eps)
