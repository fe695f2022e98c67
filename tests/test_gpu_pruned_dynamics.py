"""GPU: the second-order dynamics entries (dsge_simulate_pruned_batched, dsge_girf_pruned_batched; csrc/dsge_pruned.hpp) against
the numpy restatement of tests/pruned_dynamics_reference.py (its own deviation from ``oracle.second_order.simulate_pruned``:
<= 1e-15 of scale, bar 1e-13, tests/test_pruned_dynamics_reference.py).

Bar: the project's 1e-9 x max|reference| per output block, separately for x, x_f, x_s and girf.  Shapes: everything inside one
tile (n 6); a second row tile, a monomial count that is no multiple of 4 and states that are not the first s variables (n 17); the
SW shape (n 40); the top size (n 64, s 24, k 12); more shocks than states (n 20, s 3, k 5)."""

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

from tests import pruned_dynamics_reference as pr

pytestmark = pytest.mark.gpu

BAR = 1e-9
NAMES = list(pr.SHAPES)
KEYS = ("T", "R", "g_yy", "g_yu", "g_uu", "g_ss", "S")


def _err(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def _report(what, *errs):
    print(what, " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= BAR, (what, errs)


def _pick(x, i, per_path_ndim):
    """Draw i of an array that is shared (``per_path_ndim`` axes) or per draw."""
    return x if x.ndim == per_path_ndim else x[i]


def _sim_ref(c, eps, n_steps, x0):
    nb, n_paths, n = c["T"].shape[0], eps.shape[-3], c["T"].shape[1]
    xf, xs = np.empty((nb, n_paths, n_steps, n)), np.empty((nb, n_paths, n_steps, n))
    for i in range(nb):
        T, R, sol = pr.draw(c, i)
        for p in range(n_paths):
            start = None if x0 is None else (_pick(x0[0], i, 2)[p], _pick(x0[1], i, 2)[p])
            xf[i, p], xs[i, p] = pr.simulate_pruned(T, R, sol, _pick(eps, i, 3)[p], n_steps, start)
    return xf, xs


def _girf_ref(c, n_steps, impulses, eps, x0):
    parts = []
    for i in range(c["T"].shape[0]):
        T, R, sol = pr.draw(c, i)
        parts.append(pr.girf_pruned(T, R, sol, n_steps, None if impulses is None else _pick(impulses, i, 2),
                                    None if eps is None else _pick(eps, i, 3),
                                    None if x0 is None else (_pick(x0[0], i, 2), _pick(x0[1], i, 2))))
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def _inputs(c, rng, n_paths, n_shock, eps_batched, x0_mode):
    nb, n, k = c["R"].shape
    eps = rng.standard_normal((nb, n_paths, n_shock, k) if eps_batched else (n_paths, n_shock, k))
    eps = eps * (c["sigma"][:, None, None, :] if eps_batched else c["sigma"][0])
    if x0_mode is None:
        return eps, None
    shape = (n_paths, n) if x0_mode == "shared" else (nb, n_paths, n)
    return eps, (rng.normal(0, 0.01, shape), rng.normal(0, 0.001, shape))


# (n_paths, n_shock_steps, n_steps, eps per draw, x0): 1 / 2 / 40 steps with as many shocks and with fewer; 1, 16 and 17 paths
SIM_CASES = ((1, 1, 1, False, None), (16, 2, 2, True, "shared"), (17, 40, 40, False, "batched"), (17, 1, 2, True, None),
             (16, 25, 40, False, None), (1, 1, 2, True, "batched"))


@pytest.mark.parametrize("name", NAMES)
def test_simulate_parity(name):
    """x, x_f and x_s each within 1e-9 of their own scale; x == x_f + x_s to the LAST BIT (the kernel stores the two parts and
    their float64 sum; nothing is rounded twice)."""
    c = pr.case(name)
    sol = pr.solution(c)
    rng = np.random.default_rng(7)
    errs = []
    for n_paths, n_shock, n_steps, eps_b, x0_mode in SIM_CASES:
        eps, x0 = _inputs(c, rng, n_paths, n_shock, eps_b, x0_mode)
        out = batched.simulate_pruned_batched(sol, eps, n_steps=n_steps, x0=x0, parts=True)
        assert set(out) == {"x", "x_f", "x_s"} and out["x"].shape == (3, n_paths, n_steps, c["T"].shape[1])
        assert_array_equal(out["x"], out["x_f"] + out["x_s"])
        rf, rs = _sim_ref(c, eps, n_steps, x0)
        errs += [_err(out["x"], rf + rs), _err(out["x_f"], rf), _err(out["x_s"], rs)]
        alone = batched.simulate_pruned_batched(*(sol[key] for key in KEYS), eps, n_steps, x0)
        assert set(alone) == {"x"}
        assert_array_equal(alone["x"], out["x"])
    _report(f"simulate_pruned {name}", *errs)


@pytest.mark.parametrize("name", NAMES)
def test_girf_parity(name):
    """impulses None / shared (k, 3) / per draw (k, 1); eps None, 1, 16 and 17 baseline paths; the x_f part through the public API:
    girf - impulse_response_batched against the reference's x_s part, at 1e-9 of THAT part's scale."""
    c = pr.case(name)
    sol = pr.solution(c)
    nb, n, k = c["R"].shape
    rng = np.random.default_rng(9)
    size = c["sigma"].mean()
    errs = []
    for impulses, n_paths, n_steps, eps_b, x0_mode in ((None, 0, 40, False, None), (rng.standard_normal((k, 3)) * size, 16, 9, True, None),
                                                       (rng.standard_normal((nb, k, 1)) * size, 17, 6, False, "shared"),
                                                       (None, 1, 2, False, "batched"), (-np.eye(k)[:, :1] * size, 0, 1, False, None)):
        eps, x0 = (None, None) if n_paths == 0 else _inputs(c, rng, n_paths, min(4, n_steps), eps_b, x0_mode)
        got = batched.girf_pruned_batched(sol, n_steps=n_steps, impulses=impulses, eps=eps, x0=x0)["girf"]
        gf, gs = _girf_ref(c, n_steps, impulses, eps, x0)
        assert got.shape == gf.shape
        linear = batched.impulse_response_batched(c["T"], c["R"], n_steps=n_steps, S=impulses)["irf"]
        errs += [_err(got, gf + gs), _err(got - linear, gs)]
    _report(f"girf_pruned {name}", *errs)


def test_two_identical_calls_are_bit_identical():
    c = pr.case("n40")
    sol = pr.solution(c)
    eps, x0 = _inputs(c, np.random.default_rng(3), 17, 5, True, "shared")
    a = batched.simulate_pruned_batched(sol, eps, n_steps=8, x0=x0, parts=True)
    b = batched.simulate_pruned_batched(sol, eps, n_steps=8, x0=x0, parts=True)
    for key in ("x", "x_f", "x_s"):
        assert_array_equal(a[key], b[key])
    g = [batched.girf_pruned_batched(sol, n_steps=8, eps=eps, x0=x0)["girf"] for _ in range(2)]
    assert np.isfinite(g[0]).all()
    assert_array_equal(g[0], g[1])


@pytest.mark.parametrize("name", ["n17", "n40"])
def test_failed_draw_is_nan_and_leaves_its_neighbours_alone(name):
    c = pr.case(name)
    sol = pr.solution(c)
    eps, x0 = _inputs(c, np.random.default_rng(5), 17, 3, True, "batched")
    status = np.array([0, 1, 0], dtype=np.int32)
    clean = batched.simulate_pruned_batched(sol, eps, n_steps=5, x0=x0, status=None, parts=True)
    mixed = batched.simulate_pruned_batched(sol, eps, n_steps=5, x0=x0, status=status, parts=True)
    g_clean = batched.girf_pruned_batched(sol, n_steps=5, eps=eps, x0=x0)["girf"]
    g_mixed = batched.girf_pruned_batched(sol, n_steps=5, eps=eps, x0=x0, status=status)["girf"]
    for a, b in [(clean[key], mixed[key]) for key in ("x", "x_f", "x_s")] + [(g_clean, g_mixed)]:
        assert np.isfinite(a).all()
        assert np.isnan(b[1]).all()
        assert_array_equal(a[[0, 2]], b[[0, 2]])
    assert_array_equal(status, [0, 1, 0])  # an input


@pytest.mark.parametrize("n,s,k", [(65, 3, 2), (40, 25, 2), (20, 3, 13)])
def test_sizes_beyond_the_solver_are_refused_and_nothing_is_touched(n, s, k):
    sol = dict(T=np.zeros((2, n, n)), R=np.zeros((2, n, k)), g_yy=np.zeros((2, n, s, s)), g_yu=np.zeros((2, n, s, k)),
               g_uu=np.zeros((2, n, k, k)), g_ss=np.zeros((2, n)), S=np.arange(s))
    eps = np.zeros((2, 3, k))
    x = np.full((2, 2, 3, n), 7.0)
    with pytest.raises(_lib.DsgeTooLargeError) as e:
        F.simulate_pruned(F.HOST, sol, eps, n_steps=None, x0=None, status=None, parts=False, out=dict(x=x))
    assert e.value.code == _lib.ERR_TOO_LARGE
    g = np.full((2, k, 3, n), 7.0)
    with pytest.raises(_lib.DsgeTooLargeError):
        F.girf_pruned(F.HOST, sol, n_steps=3, impulses=None, eps=eps, x0=None, status=None, out=g)
    assert (x == 7.0).all() and (g == 7.0).all()


def test_the_solution_of_the_second_order_entry_feeds_the_simulation():
    """The dict of ``second_order_logp_batched(..., return_solution=True)`` goes straight in.  Expected: the numpy reference on THOSE
    device coefficients -- this tests the layouts, it does not compound the solver's error."""
    from tests.test_gpu_second_order import _small_batch

    n, ns, nl, k, nb = 12, 5, 4, 3, 3
    A, B, C, D, idx, val = _small_batch(n, ns, nl, k, nb, 3100 + n)
    rng = np.random.default_rng(n)
    q = rng.uniform(0.5e-4, 4e-4, (nb, k))
    Z = np.zeros((3, n))
    Z[np.arange(3), [0, 1, 7]] = 1.0
    y = rng.normal(0, 0.02, (20, 3))
    out = batched.second_order_logp_batched(A, B, C, D, idx, val, q, Z, y, Hdiag=np.full(3, 1e-5), tol=1e-12, return_solution=True)
    assert (out["status"] == 0).all(), out["status"]
    eps = rng.standard_normal((nb, 5, 7, k)) * np.sqrt(q)[:, None, None, :]
    got = batched.simulate_pruned_batched(out, eps, n_steps=10, status=out["status"], parts=True)
    girf = batched.girf_pruned_batched(out, n_steps=10, eps=eps)["girf"]
    c = dict(out, sigma=np.sqrt(q))
    rf, rs = _sim_ref(c, eps, 10, None)
    gf, gs = _girf_ref(c, 10, None, eps, None)
    _report("chain", _err(got["x"], rf + rs), _err(got["x_f"], rf), _err(got["x_s"], rs), _err(girf, gf + gs))


def test_device_front_end_equals_the_host_twins_bit_for_bit():
    import torch

    from geconpy_amd.engine import LogpEngine

    c = pr.case("n17")
    sol = pr.solution(c)
    nb, n, k = c["R"].shape
    rng = np.random.default_rng(13)
    eps, x0 = _inputs(c, rng, 17, 4, True, "shared")
    imp = rng.standard_normal((k, 2)) * 0.01
    host = batched.simulate_pruned_batched(sol, eps, n_steps=7, x0=x0, parts=True)
    host_g = batched.girf_pruned_batched(sol, n_steps=7, impulses=imp, eps=eps, x0=x0)["girf"]
    eng = LogpEngine(0)
    dsol = {key: eng.to_device(np.array(sol[key])) for key in KEYS if key != "S"}
    dsol["S"] = sol["S"]
    deps, dx0, dimp = eng.to_device(eps), tuple(eng.to_device(v) for v in x0), eng.to_device(imp)
    dev = eng.simulate_pruned(dsol, deps, n_steps=7, x0=dx0, parts=True)
    dev_g = eng.girf_pruned(*(dsol[key] for key in KEYS), 7, dimp, deps, dx0)["girf"]
    torch.cuda.synchronize()
    for key in ("x", "x_f", "x_s"):
        assert_array_equal(dev[key].cpu().numpy(), host[key])
    assert_array_equal(dev_g.cpu().numpy(), host_g)
