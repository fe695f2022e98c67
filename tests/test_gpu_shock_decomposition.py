"""GPU: the historical shock decomposition (dsge_shock_decomposition_batched; csrc/dsge_shock_decomp.hpp) against the numpy
restatement of tests/shock_decomposition_reference.py (one recursion per component; held to the convolution form at 1e-13 by
tests/test_shock_decomposition_reference.py).

Bar: the project's 1e-9, per output block and draw, on error / max|x| of the draw's input states -- no floor at 1: the states here
are about 0.05.  Every case prints its largest error."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched

from tests import shock_decomposition_cases as sc
from tests import shock_decomposition_reference as sdr
from tests import smoother_cases

pytestmark = pytest.mark.gpu

BAR = 1e-9
UNEVEN = [[0, 1], [2, 6], [3, 4, 5]]  # group_of_shock = [0, 0, 1, 2, 2, 2, 1]


def _paths(T, R, n_paths, T_len, seed=0):
    e = sc.shocks(T.shape[0], n_paths, T_len, R.shape[2], seed)
    return sc.exact_paths(T, R, e, seed), e


def _errors(got, ref, x):
    """Largest error / max|x| per output block, over the draws."""
    errs = {}
    for key in ("contributions", "observed"):
        assert (got[key] is None) == (ref[key] is None), key
        if ref[key] is not None:
            assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
            errs[key] = max(np.abs(got[key][b] - ref[key][b]).max() / np.abs(x[b]).max() for b in range(x.shape[0]))
    return errs


def _check(what, T, R, x, e, **kw):
    got = batched.shock_decomposition_batched(T, R, x, e, **kw)
    if x.ndim == 3:  # the smoother's layout: one path, no path axis
        ref = {key: None if v is None else v[:, 0] for key, v in sdr.batch_decomposition(T, R, x[:, None], e[:, None], **kw).items()}
    else:
        ref = sdr.batch_decomposition(T, R, x, e, **kw)
    if ref["contributions"].shape[-2] == 0:  # no variable asked for
        ref["contributions"] = None
    errs = _errors(got, ref, x)
    print(what, " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert errs and max(errs.values()) <= BAR, (what, errs)
    return got


# ---- tile and LDS edges, sample edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, m", [("rbc", 8), ("sw16", 16), ("sw17", 17), ("full_nk", 24), ("sw40", 40), ("sw49", 49), ("sw64", 64),
                                     ("sw96", 96)])
def test_tile_and_lds_edges(name, m):
    """Identity groups (rbc: k = 1, G = 2), three distinct draws, two paths, 40 periods, every variable and a dense Z."""
    T, R = sc.model(name)
    assert T.shape == (3, m, m) and not (T[0] == T[1]).all() and not (T[1] == T[2]).all()
    x, e = _paths(T, R, 2, 40)
    Z = np.random.default_rng(m).standard_normal((3, m))
    got = _check(f"edges {name}", T, R, x, e, Z=Z)
    k = R.shape[2]
    assert got["components"] == [*range(k), "initial", "remainder"]
    assert got["contributions"].shape == (3, 2, 40, m, k + 2) and got["observed"].shape == (3, 2, 40, 3, k + 2)


@pytest.mark.parametrize("T_len", [1, 2, 3])
def test_short_samples(T_len):
    """T_len = 1: the initial condition alone, nothing multiplied, the shocks (one NaN period) never read."""
    T, R = sc.model("sw17")
    x, e = _paths(T, R, 2, T_len, seed=T_len)
    got = _check(f"T_len {T_len}", T, R, x, e, Z=np.eye(2, 17))
    c0 = got["contributions"][:, :, 0]
    assert (c0[..., :3] == 0).all() and (c0[..., 4] == 0).all()
    assert_array_equal(c0[..., 3], x[:, :, 0])


def test_smoother_layout_is_the_one_path_case():
    """(batch, T_len, .) inputs: the outputs lose the path axis and equal the 4-d call bit for bit."""
    T, R = sc.model("sw17")
    x, e = _paths(T, R, 1, 6)
    four = batched.shock_decomposition_batched(T, R, x, e, Z=np.eye(2, 17))
    three = batched.shock_decomposition_batched(T, R, x[:, 0], e[:, 0], Z=np.eye(2, 17))
    assert three["contributions"].shape == (3, 6, 17, 5) and three["observed"].shape == (3, 6, 2, 5)
    assert_array_equal(three["contributions"], four["contributions"][:, 0])
    assert_array_equal(three["observed"], four["observed"][:, 0])


# ---- components ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, name, groups", [
    ("one group", "sw40", [list(range(7))]),
    ("uneven", "sw40", UNEVEN),
    ("k = 15, identity: G = 16 fills the tile", "wide20_15", None),
    ("k = 16 in two groups", "wide20_16", [list(range(0, 16, 2)), list(range(1, 16, 2))]),
    ("k = 16 in 15 groups", "wide20_16", [[j] for j in range(14)] + [[14, 15]]),
])
def test_groups(what, name, groups):
    T, R = sc.model(name)
    x, e = _paths(T, R, 2, 12)
    got = _check(what, T, R, x, e, groups=groups, Z=np.random.default_rng(5).standard_normal((2, T.shape[1])))
    g = R.shape[2] if groups is None else len(groups)
    assert got["components"] == [*range(g), "initial", "remainder"]


def test_sixteen_groups_are_refused():
    T, R = sc.model("wide20_16")
    x, e = _paths(T, R, 1, 3)
    with pytest.raises(_lib.DsgeTooLargeError, match="15 groups") as info:
        batched.shock_decomposition_batched(T, R, x, e)
    assert info.value.code == _lib.ERR_TOO_LARGE


# ---- paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_paths", [1, 2, 3, 17])
@pytest.mark.parametrize("name", ["rbc", "sw40"])
def test_paths(name, n_paths):
    """rbc: G = 2, eight paths share a tile (17 paths: packs of 8, 8, 1); sw40: G = 8, two paths share it (3 paths: 2, 1).  Z
    shared and per draw."""
    T, R = sc.model(name)
    m = T.shape[1]
    x, e = _paths(T, R, n_paths, 5, seed=n_paths)
    rng = np.random.default_rng(n_paths)
    _check(f"paths {name} {n_paths} shared Z", T, R, x, e, Z=rng.standard_normal((2, m)))
    _check(f"paths {name} {n_paths} per-draw Z", T, R, x, e, Z=rng.standard_normal((3, 2, m)))


# ---- selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sw17", "sw40"])
def test_selection(name):
    T, R = sc.model(name)
    m = T.shape[1]
    x, e = _paths(T, R, 3, 7)
    rng = np.random.default_rng(m)
    for variables in (None, [5, 0, m - 1], [3]):
        got = _check(f"selection {name} {variables}", T, R, x, e, variables=variables)
        assert got["observed"] is None
    for p in (1, 3, 16):
        _check(f"selection {name} p = {p}", T, R, x, e, variables=[5, 0, m - 1], Z=rng.standard_normal((p, m)), groups=UNEVEN
               if name == "sw40" else None)
    got = _check(f"selection {name} observed only", T, R, x, e, variables=(), Z=rng.standard_normal((3, m)))
    assert got["contributions"] is None and got["observed"].shape == (3, 3, 7, 3, R.shape[2] + 2)


# ---- remainder -----------------------------------------------------------------------------------------------------------------
def test_remainder():
    T, R = sc.model("sw40")
    x, e = _paths(T, R, 3, 40)
    Z = np.random.default_rng(1).standard_normal((3, 40))
    exact = _check("remainder, exact path", T, R, x, e, groups=UNEVEN, Z=Z)
    scale = np.abs(x).reshape(3, -1).max(axis=1)[:, None, None, None]
    rel = np.abs(exact["contributions"][..., -1]) / scale
    print(f"remainder on an exact path / max|x|: {rel.max():.2e}")
    assert rel.max() <= 1e-12
    # a known perturbation of x comes back as the remainder; period 0 is the initial condition, so its remainder stays 0
    delta = 1e-3 * np.random.default_rng(2).standard_normal(x.shape)
    delta[:, :, 0] = 0.0
    moved = _check("remainder, perturbed path", T, R, x + delta, e, groups=UNEVEN, Z=Z)
    err = np.abs(moved["contributions"][..., -1] - delta) / scale
    print(f"remainder - perturbation / max|x|: {err.max():.2e}")
    assert err.max() <= BAR
    assert (moved["contributions"][:, :, 0, :, -1] == 0).all()
    assert_array_equal(moved["contributions"][..., :-1], exact["contributions"][..., :-1])
    # without the remainder the other components are the same bits
    bare = _check("remainder off", T, R, x, e, groups=UNEVEN, Z=Z, remainder=False)
    assert bare["components"] == [0, 1, 2, "initial"]
    assert_array_equal(bare["contributions"], exact["contributions"][..., :-1])
    assert_array_equal(bare["observed"], exact["observed"][..., :-1])
    # with it the components add up to x and to Z x
    total = np.abs(exact["contributions"].sum(axis=-1) - x) / scale
    total_obs = np.abs(exact["observed"].sum(axis=-1) - np.einsum("pi,bsti->bstp", Z, x)) / scale
    print(f"sum of components - x: {total.max():.2e}, - Z x: {total_obs.max():.2e}")
    assert total.max() <= 1e-12 and total_obs.max() <= 1e-12


# ---- e[0] is ignored, NaN containment ------------------------------------------------------------------------------------------
def test_first_period_shocks_are_never_read():
    T, R = sc.model("sw17")
    x, e = _paths(T, R, 3, 6)
    Z = np.eye(2, 17)
    assert np.isnan(e[:, :, 0]).all()
    nan = batched.shock_decomposition_batched(T, R, x, e, Z=Z)
    assert np.isfinite(nan["contributions"]).all() and np.isfinite(nan["observed"]).all()
    big = e.copy()
    big[:, :, 0] = 1e300
    huge = batched.shock_decomposition_batched(T, R, x, big, Z=Z)
    assert_array_equal(huge["contributions"], nan["contributions"])
    assert_array_equal(huge["observed"], nan["observed"])


@pytest.mark.parametrize("name, n_paths", [("sw40", 3), ("rbc", 9)])
def test_nan_stays_in_its_path(name, n_paths):
    """A NaN in e[t >= 1] of one path: NaN from step t on in that path (in the shock's group and in the remainder; the other
    groups never see the shock), every other path and draw bit-identical to the clean call."""
    T, R = sc.model(name)
    x, e = _paths(T, R, n_paths, 8)
    Z = np.random.default_rng(4).standard_normal((2, T.shape[1]))
    clean = batched.shock_decomposition_batched(T, R, x, e, Z=Z)
    bad = e.copy()
    bad[1, 1, 3, 0] = np.nan
    got = batched.shock_decomposition_batched(T, R, x, bad, Z=Z)
    for key in ("contributions", "observed"):
        hit = np.zeros(got[key].shape[:2], dtype=bool)
        hit[1, 1] = True
        assert_array_equal(got[key][~hit], clean[key][~hit], err_msg=key)
        assert_array_equal(got[key][1, 1, :3], clean[key][1, 1, :3], err_msg=key)
        assert np.isnan(got[key][1, 1, 3:, :, 0]).all() and np.isnan(got[key][1, 1, 3:, :, -1]).all(), key
        assert_array_equal(got[key][1, 1, :, :, 1:-1], clean[key][1, 1, :, :, 1:-1], err_msg=key)


# ---- chains on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sw17_qfull", "zc48"])
def test_smoother_chain(name):
    c = smoother_cases.case(name)
    args = (c["T"], c["R"], c["q"], c["Z"], c["y"])
    kw = dict(d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"])
    s = batched.kalman_smoother_batched(*args, **kw)
    assert (s["status"] == 0).all()
    x, e = s["smoothed_states"], s["smoothed_shocks"]
    got = _check(f"chain {name}", c["T"], c["R"], x[:, None], e[:, None], Z=c["Z"])
    scale = np.abs(x).reshape(x.shape[0], -1).max(axis=1)[:, None, None]
    total = np.abs(got["contributions"][:, 0].sum(axis=-1) - x) / scale
    rem = np.abs(got["contributions"][:, 0, :, :, -1]) / scale
    print(f"chain {name}, default conventions: sum - x {total.max():.2e}, remainder {rem.max():.2e} of max|x|")
    assert total.max() <= 1e-12
    s = batched.kalman_smoother_batched(*args, **kw, options=_lib.filter_conventions(jitter_on_P=False))
    assert (s["status"] == 0).all()
    x, e = s["smoothed_states"], s["smoothed_shocks"]
    got = _check(f"chain {name}, jitter_on_P=False", c["T"], c["R"], x, e)
    scale = np.abs(x).reshape(x.shape[0], -1).max(axis=1)[:, None, None]
    rem = np.abs(got["contributions"][..., -1]) / scale
    print(f"chain {name}, jitter_on_P=False: remainder {rem.max():.2e} of max|x|")
    assert rem.max() <= 1e-10


def test_simulation_smoother_chain():
    c = smoother_cases.case("sw17_qfull")
    s = batched.simulation_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], n_paths=3, d=c["d"], Hdiag=c["H"],
                                            q_mode=c["q_mode"], rng=11)
    assert (s["status"] == 0).all() and s["states"].shape[:3] == (2, 3, smoother_cases.N_STEPS)
    assert np.isnan(s["shocks"][:, :, 0]).all()
    got = _check("chain simulation smoother", c["T"], c["R"], s["states"], s["shocks"], Z=c["Z"])
    scale = np.abs(s["states"]).reshape(2, -1).max(axis=1)[:, None, None, None]
    assert (np.abs(got["contributions"].sum(axis=-1) - s["states"]) / scale).max() <= 1e-12


# ---- determinism and dispatch --------------------------------------------------------------------------------------------------
def test_failed_draw_does_not_disturb_the_batch():
    T, R = sc.model("sw40")
    x, e = _paths(T, R, 3, 9)
    Z = np.random.default_rng(6).standard_normal((2, 40))
    status = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32)
    poisoned_T = T.copy()
    poisoned_T[1] = np.nan
    out = batched.shock_decomposition_batched(poisoned_T, R, x, e, Z=Z, status=status)
    for key in ("contributions", "observed"):
        assert np.isnan(out[key][1]).all(), key
    for i in (0, 2):
        one = batched.shock_decomposition_batched(T[i:i + 1], R[i:i + 1], x[i:i + 1], e[i:i + 1], Z=Z)
        for key in ("contributions", "observed"):
            assert np.isfinite(one[key]).all()
            assert_array_equal(out[key][i], one[key][0], err_msg=key)


def test_two_calls_give_the_same_bits():
    T, R = sc.model("sw49")
    x, e = _paths(T, R, 3, 20)
    Z = np.random.default_rng(7).standard_normal((3, 3, 49))
    one = batched.shock_decomposition_batched(T, R, x, e, groups=UNEVEN, Z=Z)
    two = batched.shock_decomposition_batched(T, R, x, e, groups=UNEVEN, Z=Z)
    for key in ("contributions", "observed"):
        assert_array_equal(one[key], two[key], err_msg=key)


def test_engine_equals_host_twin():
    import torch

    from geconpy_amd.engine import LogpEngine

    T, R = sc.model("sw40")
    x, e = _paths(T, R, 3, 10)
    Z = np.random.default_rng(8).standard_normal((2, 40))
    host = batched.shock_decomposition_batched(T, R, x, e, groups=UNEVEN, variables=[5, 0, 39], Z=Z)
    eng = LogpEngine(0)
    dev = eng.shock_decomposition(*(eng.to_device(np.array(a)) for a in (T, R, x, e)), groups=UNEVEN, variables=[5, 0, 39], Z=eng.to_device(Z))
    torch.cuda.synchronize()
    assert dev["components"] == host["components"] == [0, 1, 2, "initial", "remainder"]
    for key in ("contributions", "observed"):
        assert_array_equal(dev[key].cpu().numpy(), host[key], err_msg=key)
    # preallocated outputs are filled in place
    out = dict(contributions=torch.empty_like(dev["contributions"]), observed=torch.empty_like(dev["observed"]))
    again = eng.shock_decomposition(*(eng.to_device(np.array(a)) for a in (T, R, x, e)), groups=UNEVEN, variables=[5, 0, 39], Z=eng.to_device(Z),
                                    out=out)
    torch.cuda.synchronize()
    assert again["contributions"] is out["contributions"] and torch.equal(out["contributions"], dev["contributions"])
    assert torch.equal(out["observed"], dev["observed"])
