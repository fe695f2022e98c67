"""GPU: the device smoother (dsge_kalman_smoother_batched, csrc/dsge_kalman_smooth.hpp) against the numpy restatement of the
upstream recursion (tests/smoother_reference.py::rts_smoother on oracle.kalman_filter_logp(..., return_states=True)).

Bar: the project's per-step-output bar, 1e-9 x scale, with sc = max(1, |a_filt|max) for states, pc = |P_pred|max for
covariances, ec = max sqrt(Q_jj) for shocks.  The reference's own noise is <= 2e-11 (docs/design/smoother.md)."""
import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import oracle
from geconpy_amd import _lib, batched
from geconpy_amd import workloads as wl

from tests import smoother_cases as cases
from tests.smoother_reference import rts_smoother

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _solve(b, nb):
    T = np.empty_like(b["A"][:nb])
    for i in range(nb):
        T[i], ok, _ = oracle.cycle_reduction.cycle_reduction_core(b["A"][i], b["B"][i], b["C"][i], 1000, 1e-12)
        assert ok
    R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(nb)])
    return T, R


def _missing(y):
    y = y.copy()
    y[5, min(1, y.shape[1] - 1)] = np.nan
    y[11] = np.nan
    y[-1, 0] = np.nan
    return y


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(T, R, q, q_mode, Z, y, d, H): the inputs of one parity case (computed once, shared, never modified); the edge cases
    come from tests/smoother_cases.py, which the CPU test of the two numpy forms reads too."""
    if name in cases.ALL_CASES:
        return cases.case(name)
    rng = np.random.default_rng(5)
    d = None
    if name == "rbc":
        b, om = wl.rbc_batch(3)
        T, R = _solve(b, 3)
        Z, H, y = om["Z"], np.zeros(1), _missing(om["y"][:12])
    elif name == "full_nk":
        b, _ = wl.full_nk_batch(3)
        T, R = _solve(b, 3)
        m = T.shape[1]
        is_state = np.abs(T[0]).sum(axis=0) > 0
        Z = np.zeros((2, m))
        Z[0, np.flatnonzero(is_state)[0]] = 1.0
        Z[1, np.flatnonzero(~is_state)[0]] = 1.0
        H, y = np.full(2, 1e-6), _missing(np.random.default_rng(0).normal(0, 0.01, (12, 2)))
    elif name in ("sw", "sw_dense", "sw_singular"):
        b = wl.sw_shaped_batch(4)
        om = wl.sw_shaped_observation_model()
        T = b["T_star"]
        R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(4)])
        if name == "sw_singular":
            Z, H, y = om["Z"], np.zeros(7), om["y"][:30].copy()
        else:
            Z, H, y = om["Z"][:4].copy(), np.full(4, 1e-5), _missing(om["y"][:30, :4])
            if name == "sw_dense":
                Z = Z + 0.05 * rng.standard_normal(Z.shape) * (rng.random(Z.shape) < 0.2)
                d = rng.normal(0, 0.01, 4)
    elif name in ("sw17", "sw64"):
        sh = dict(n=17, n_state=7, n_lead=5, k=3) if name == "sw17" else dict(n=64, n_state=30, n_lead=20, k=8)
        b = wl.sw_shaped_batch(2, **sh)
        T = b["T_star"]
        R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(2)])
        Z, H = np.eye(4, sh["n"]), np.full(4, 1e-5)
        x = np.zeros(sh["n"])
        y = np.empty((30, 4))
        for t in range(30):  # (a panel simulated from draw 0)
            x = T[0] @ x + R[0] @ (rng.standard_normal(sh["k"]) * b["sigma"][0])
            y[t] = Z @ x + rng.standard_normal(4) * np.sqrt(H)
        y = _missing(y)
    else:
        raise KeyError(name)
    q = b["sigma"][: T.shape[0]] ** 2
    for a in (T, R, q, Z, y, H):
        a.setflags(write=False)
    return dict(T=T, R=R, q=q, q_mode="diag_batched", Z=Z, y=y, d=d, H=H)


@functools.lru_cache(maxsize=None)
def _reference(name, conv=None):
    c = _case(name)
    cv = None if conv is None else oracle.FilterConventions(**dict(conv))
    out = []
    for i in range(c["T"].shape[0]):
        x = cases.draw(c, i)  # (the matrices of draw i: Q as (k, k), Z, d, H of the draw where they are given per draw)
        _, ll, stt = oracle.kalman_filter_logp(c["y"], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"],
                                               return_states=True, conventions=cv)
        out.append((ll, stt) + rts_smoother(stt, x["T"], x["R"], x["Q"]))
    return out


def _run(name, **kw):
    c = _case(name)
    return batched.kalman_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"], **kw)


def _check_parity(name, conv=None, options=None, guard=False):
    c = _case(name)
    full = _run(name, full_covariances=True, options=options)
    diag = _run(name, options=options)
    assert (full["status"] == 0).all() and (diag["status"] == 0).all()
    assert np.isnan(full["smoothed_shocks"][:, 0]).all() and np.isnan(diag["smoothed_shocks"][:, 0]).all()
    assert_array_equal(full["smoothed_states"], diag["smoothed_states"])
    assert_array_equal(np.diagonal(full["smoothed_covs"], axis1=2, axis2=3), diag["smoothed_covs"])
    for i, (ll, stt, a, V, e) in enumerate(_reference(name, conv)):
        sc, pc, ec = cases.scales(c, i, stt)  # max(1, |a_filt|max), |P_pred|max, max sqrt(Q_jj)
        errs = (np.abs(full["smoothed_states"][i] - a).max() / sc, np.abs(full["smoothed_covs"][i] - V).max() / pc,
                np.abs(full["smoothed_shocks"][i, 1:] - e[1:]).max() / ec)
        print(name, i, "errors / scale (states, covs, shocks):", errs)
        assert_allclose(full["ll"][i], ll, rtol=1e-8, atol=1e-9)
        assert_allclose(full["smoothed_states"][i], a, rtol=0, atol=BAR * sc)
        assert_allclose(full["smoothed_covs"][i], V, rtol=0, atol=BAR * pc)
        assert_allclose(full["smoothed_shocks"][i, 1:], e[1:], rtol=0, atol=BAR * ec)
        if guard:  # smoothing is not trivially the filter
            assert np.abs(a - stt["a_filt"]).max() / sc > 1e-2
    return full


@pytest.mark.parametrize("name", ["rbc", "full_nk", "sw", "sw_dense"])
def test_parity_real_models(name):
    """States, full and diagonal covariances, shocks from t >= 1 (shocks[:, 0] = NaN) on RBC (m = 8), full_nk (m = 24, rank-
    deficient [T | R]) and SW-shaped draws (m = 40; selector Z, and dense Z + d), with a partial-missing row, an empty row and a
    missing entry in the last row; the per-step ll sums to kalman_logp_batched."""
    c = _case(name)
    out = _check_parity(name, guard=True)
    lp, st = batched.kalman_logp_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], d=c["d"], Hdiag=c["H"])
    assert (st == 0).all()
    assert_allclose(out["ll"].sum(axis=1), lp, rtol=1e-10)


@pytest.mark.parametrize("name", ["sw17", "sw64"])
def test_parity_padding_and_lds_split(name):
    """m = 17 (one variable past a 16-wide tile, r = 10) and m = 64 (U and U'T read from global memory, r = 38)."""
    _check_parity(name)


def test_parity_stochastically_singular():
    """All seven observables without measurement error: P_filt at jitter level on the states, cond(M) ~ 2e5."""
    _check_parity("sw_singular")


def test_conventions_and_decomposition_identity():
    """The other filter conventions end to end, and -- without the P jitter, where it holds (6e-14 in numpy; 1e-5 under
    jitter_on_P, not asserted there) -- the historical decomposition as[t+1] = T as[t] + R eps[t+1]."""
    conv = dict(ll_constant="one", jitter_on_F=True, jitter_on_P=False, mask_d=True, joseph=False)
    out = _check_parity("sw", conv=tuple(sorted(conv.items())), options=_lib.filter_conventions(**conv))
    c = _case("sw")
    for i, (_, stt, _, _, _) in enumerate(_reference("sw", tuple(sorted(conv.items())))):
        a, e = out["smoothed_states"][i], out["smoothed_shocks"][i]
        resid = a[1:] - a[:-1] @ c["T"][i].T - e[1:] @ c["R"][i].T
        sc = max(1.0, np.abs(stt["a_filt"]).max())
        print("decomposition residual / sc:", np.abs(resid).max() / sc)
        assert np.abs(resid).max() <= 1e-10 * sc


def test_failed_draw_does_not_disturb_the_batch():
    c = _case("sw")
    status = np.zeros(4, dtype=np.int32)
    status[1] = _lib.ST_NOT_CONVERGED
    out = batched.kalman_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], Hdiag=c["H"], status=status, full_covariances=True)
    assert out["status"].tolist() == [0, _lib.ST_NOT_CONVERGED, 0, 0]
    for key in ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks"):
        assert np.isnan(out[key][1]).all(), key
    for i in (0, 2, 3):
        one = batched.kalman_smoother_batched(c["T"][i:i + 1], c["R"][i:i + 1], c["q"][i:i + 1], c["Z"], c["y"], Hdiag=c["H"],
                                              full_covariances=True)
        assert one["status"][0] == 0
        for key in ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks"):
            assert_array_equal(out[key][i], one[key][0], err_msg=key)


def test_chunked_equals_unchunked():
    """Batch 8 at m = 17, 12 steps, scratch for exactly 3 draws (chunks of 3, 3, 2): bit-identical to one chunk."""
    sh = dict(n=17, n_state=7, n_lead=5, k=3)
    b = wl.sw_shaped_batch(8, **sh)
    T = b["T_star"]
    R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(8)])
    c = _case("sw17")
    args = (T, R, b["sigma"] ** 2, c["Z"], c["y"][:12])
    one = batched.kalman_smoother_batched(*args, Hdiag=c["H"], full_covariances=True)
    three = batched.kalman_smoother_batched(*args, Hdiag=c["H"], full_covariances=True,
                                            scratch_limit_bytes=3 * batched.smoother_scratch_bytes_per_draw(17, 12))
    tiny = batched.kalman_smoother_batched(*args, Hdiag=c["H"], full_covariances=True, scratch_limit_bytes=1)
    assert (one["status"] == 0).all()
    assert np.isfinite(one["smoothed_covs"]).all()
    for key in ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks", "status"):
        assert_array_equal(one[key], three[key], err_msg=key)
        assert_array_equal(one[key], tiny[key], err_msg=key)


def test_chunked_equals_unchunked_every_member_batched():
    """The same chunks (3, 3, 2) with Z, d, Hdiag and a full Q given per draw, all different from draw to draw: bit-identical to
    one chunk, and draws 2, 3, 5, 7 (last of a chunk, first of the next, mid-chunk, last of the batch) bit-identical to the
    one-draw call on their own slices -- which an offset that is wrong in both runs would not be."""
    sh = dict(n=17, n_state=7, n_lead=5, k=3)
    b = wl.sw_shaped_batch(8, **sh)
    T = b["T_star"]
    R = np.stack([oracle.compute_selection_matrix(b["B"][i], b["C"][i], b["D"][i], T[i]) for i in range(8)])
    c = _case("sw17")
    scale = 1.0 + np.arange(8) / 16.0
    Z = c["Z"][None] * scale[:, None, None]
    d = np.random.default_rng(8).normal(0, 0.01, (8, 4))
    H = c["H"][None] * scale[:, None] ** 2
    s = b["sigma"]
    Q = np.stack([np.diag(s[i] ** 2) + 0.1 * scale[i] * (np.outer(s[i], s[i]) - np.diag(s[i] ** 2)) for i in range(8)])
    assert all(np.linalg.eigvalsh(Q[i]).min() > 0 for i in range(8))
    y = c["y"][:12]
    kw = dict(full_covariances=True)
    keys = ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks", "status")
    one = batched.kalman_smoother_batched(T, R, Q, Z, y, d=d, Hdiag=H, **kw)
    three = batched.kalman_smoother_batched(T, R, Q, Z, y, d=d, Hdiag=H, **kw,
                                            scratch_limit_bytes=3 * batched.smoother_scratch_bytes_per_draw(17, 12))
    assert (one["status"] == 0).all() and np.isfinite(one["smoothed_covs"]).all()
    for key in keys:
        assert_array_equal(one[key], three[key], err_msg=key)
    for i in (2, 3, 5, 7):
        own = batched.kalman_smoother_batched(T[i:i + 1], R[i:i + 1], Q[i:i + 1], Z[i:i + 1], y, d=d[i:i + 1], Hdiag=H[i:i + 1], **kw)
        for key in keys:
            assert_array_equal(three[key][i], own[key][0], err_msg=f"{key}, draw {i}")


def test_edges():
    c = _case("sw")
    kw = dict(Hdiag=c["H"], full_covariances=True)
    # one step: smoothed = filtered, shocks NaN
    one = batched.kalman_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"][:1], **kw)
    filt = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["q"], c["Z"], c["y"][:1], **kw)
    assert_array_equal(one["smoothed_states"], filt["filtered_states"])
    assert_array_equal(one["smoothed_covs"], filt["filtered_covs"])
    assert_array_equal(one["ll"], filt["ll"])
    assert np.isnan(one["smoothed_shocks"]).all() and (one["status"] == 0).all()
    # no step, no draw
    e0 = batched.kalman_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"][:0], **kw)
    assert e0["smoothed_states"].shape == (4, 0, 40) and e0["smoothed_shocks"].shape == (4, 0, 7) and (e0["status"] == 0).all()
    e1 = batched.kalman_smoother_batched(np.empty((0, 40, 40)), np.empty((0, 40, 7)), np.empty((0, 7)), c["Z"], c["y"], **kw)
    assert e1["smoothed_covs"].shape == (0, 30, 40, 40) and e1["status"].shape == (0,)
    # states only through the C entry: covariance and shock pointers NULL (and ll), same states bit for bit
    ref = _run("sw")
    T, R, q, Z, y, H = (np.ascontiguousarray(c[x], dtype=np.float64) for x in ("T", "R", "q", "Z", "y", "H"))
    a = np.empty((4, 30, 40))
    st = np.zeros(4, dtype=np.int32)
    p = lambda x: x.ctypes.data  # noqa: E731
    lib = _lib.load()
    _lib.check(lib.dsge_kalman_smoother_batched_host(p(T), p(R), p(q), _lib.Q_DIAG_BATCHED, p(Z), 0, None, 0, p(H), 0, p(y), 4, 40, 7,
                                                      4, 30, 1e-8, -9999.0, 0.0, 0, None, p(a), None, None, 0, p(st)))
    assert (st == 0).all()
    assert_array_equal(a, ref["smoothed_states"])
    assert lib.dsge_kalman_smoother_batched_host(p(T), p(R), p(q), _lib.Q_DIAG_BATCHED, p(Z), 0, None, 0, p(H), 0, p(y), 4, 40, 7, 4,
                                                 30, 1e-8, -9999.0, 0.0, 0, None, None, None, None, 0, p(st)) == _lib.ERR_INVALID


def test_engine_equals_host_twin():
    import torch
    from geconpy_amd.engine import LogpEngine

    c = _case("sw")
    ref = _run("sw", full_covariances=True)
    eng = LogpEngine(0)
    dev = {x: eng.to_device(np.array(c[x])) for x in ("T", "R", "q", "Z", "y", "H")}
    out = eng.kalman_smoother(dev["T"], dev["R"], dev["q"], dev["Z"], dev["y"], Hdiag=dev["H"], q_mode=1, full_covariances=True)
    nocov = eng.kalman_smoother(dev["T"], dev["R"], dev["q"], dev["Z"], dev["y"], Hdiag=dev["H"], q_mode=1, covariances=False)
    torch.cuda.synchronize()
    assert nocov["smoothed_covs"] is None
    for key in ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks", "status"):
        assert_array_equal(out[key].cpu().numpy(), ref[key], err_msg=key)
    assert_array_equal(nocov["smoothed_states"].cpu().numpy(), ref["smoothed_states"])
    assert_array_equal(nocov["smoothed_shocks"].cpu().numpy(), ref["smoothed_shocks"])


# ---- the edges (tests/smoother_cases.py; the same inputs pass tests/test_smoother_reference.py::test_range_form_matches_pinv_form
#      at 1e-10 x scale in numpy, so a miss here is the device's) ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.ZERO_COLUMN))
def test_parity_zero_columns_at_class_boundaries(name):
    """m = 16, 32, 33, 48, 49 with r = 10, 19, 19, 29, 29: the last model of each LDS class and the first of the next (m = 48:
    seven images in LDS; m = 49: U, U'T, U'R read from global memory)."""
    _check_parity(name)


@pytest.mark.parametrize("name", list(cases.DENSE))
def test_parity_full_rank(name):
    """r = m: a dense T with [T | R] of full rank (the plain Rauch-Tung-Striebel case; rt == mt, r4 == m4, an m x m elimination
    with m right-hand sides; at m = 16, 32, 48, 64 the 16-wide tiles are full, no zero padding) -- m = 1 and 2, every class
    boundary, p = 16, k = m = 20 and k = m = 64 (lanes 64 .. 64 + k, m + k = 128 column norms in the basis kernel)."""
    _check_parity(name)


@pytest.mark.parametrize("name", list(cases.SHOCK_FORMS))
def test_parity_shock_covariance_forms(name):
    """A full Q, shared and per draw (eps = Q (R'w), the diagonal pick Q[j, j] of the basis kernel), and J = {j : Q_jj > 0} a
    proper subset, in a diagonal and in a full Q (the R column of the shock without variance leaves the basis: r = 9 instead of 10
    at m = 17), each against the reference; the shock without variance is smoothed to exactly 0."""
    c = _case(name)
    out = _check_parity(name)
    if c["zero_shock"] is not None:
        assert (out["smoothed_shocks"][:, 1:, c["zero_shock"]] == 0.0).all()


@pytest.mark.parametrize("name", ["obs_batched", "p1", "tlen2", "tlen3"])
def test_parity_observation_forms_and_short_samples(name):
    """Z, d, Hdiag and a full Q per draw against the reference, draw by draw; p = 1; T_len = 2 (one backward step, the prefetch of
    step t - 1 never runs) and 3."""
    _check_parity(name)


def _own_call(c, i, **kw):
    """Draw i of the case on its own."""
    own = lambda x, shared_ndim: x if x is None or x.ndim == shared_ndim else x[i:i + 1]  # noqa: E731
    q = c["q"][i:i + 1] if c["q_mode"].endswith("batched") else c["q"]
    return batched.kalman_smoother_batched(c["T"][i:i + 1], c["R"][i:i + 1], q, own(c["Z"], 2), c["y"], d=own(c["d"], 1),
                                           Hdiag=own(c["H"], 1), q_mode=c["q_mode"], **kw)


KEYS = ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks")


def test_singular_m_sets_the_status_and_returns():
    """DSGE_ST_SMOOTHER_SINGULAR (256), deterministically: without the P jitter the second pivot of M is exactly 0 in draw 1 at the
    first backward step (tests/smoother_cases.py).  The draw keeps its log-likelihood and its last step (= the filter's, bit for
    bit), every earlier step and every shock row is NaN; draws 0 and 2 are bit-identical to their own one-draw calls and within
    the bar of the reference.  Under the default conventions the same batch has status 0 and meets the bar in every draw."""
    name = "singular_m_nojit"
    c = _case(name)
    kw = dict(full_covariances=True, options=_lib.filter_conventions(**c["conv"]))
    out = _run(name, **kw)
    assert out["status"].tolist() == [0, _lib.ST_SMOOTHER_SINGULAR, 0]
    assert _lib.ST_SMOOTHER_SINGULAR == 256
    filt = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], Hdiag=c["H"], q_mode=c["q_mode"], **kw)
    assert (filt["status"] == 0).all()
    assert np.isfinite(out["ll"][1]).all()
    assert_array_equal(out["ll"][1], filt["ll"][1])
    assert_array_equal(out["smoothed_states"][1, -1], filt["filtered_states"][1, -1])
    assert_array_equal(out["smoothed_covs"][1, -1], filt["filtered_covs"][1, -1])
    assert np.isnan(out["smoothed_states"][1, :-1]).all() and np.isnan(out["smoothed_covs"][1, :-1]).all()
    assert np.isnan(out["smoothed_shocks"][1]).all()
    diag = _run(name, options=kw["options"])  # (the diagonal call takes the other extent of the NaN prefix)
    assert diag["status"].tolist() == [0, _lib.ST_SMOOTHER_SINGULAR, 0]
    assert_array_equal(diag["smoothed_covs"][1, -1], np.diagonal(filt["filtered_covs"][1, -1]))
    assert np.isnan(diag["smoothed_covs"][1, :-1]).all() and np.isnan(diag["smoothed_states"][1, :-1]).all()
    for i, (ll, stt, a, V, e) in cases.reference(name).items():
        own = _own_call(c, i, **kw)
        assert own["status"][0] == 0
        for key in KEYS:
            assert_array_equal(out[key][i], own[key][0], err_msg=f"{key}, draw {i}")
        assert_array_equal(diag["smoothed_states"][i], out["smoothed_states"][i])
        sc, pc, ec = cases.scales(c, i, stt)
        assert_allclose(out["ll"][i], ll, rtol=1e-8, atol=1e-9)
        assert_allclose(out["smoothed_states"][i], a, rtol=0, atol=BAR * sc)
        assert_allclose(out["smoothed_covs"][i], V, rtol=0, atol=BAR * pc)
        assert_allclose(out["smoothed_shocks"][i, 1:], e[1:], rtol=0, atol=BAR * ec)
    _check_parity("singular_m")  # default conventions: M = diag(1.3, 2.5e-9) in draw 1


def test_forward_pass_failing_on_one_draw():
    """DSGE_ST_FILTER_NONFINITE (8) set by the outputs kernel INSIDE a smoother call and read by the two smoother kernels on the
    same stream: without the F jitter, F[1, 1] is exactly 0 in draw 1 (a zero row of its Z, no measurement error).  Every smoothed
    output of that draw is NaN; draws 0 and 2 have status 0 and are bit-identical to their own one-draw calls."""
    c = _case("forward_fail")
    kw = dict(full_covariances=True, options=_lib.filter_conventions(**c["conv"]))
    out = _run("forward_fail", **kw)
    assert _lib.ST_FILTER_NONFINITE == 8
    assert out["status"][1] & _lib.ST_FILTER_NONFINITE
    assert out["status"][0] == 0 and out["status"][2] == 0
    for key in KEYS[1:]:
        assert np.isnan(out[key][1]).all(), key
    for i in (0, 2):
        own = _own_call(c, i, **kw)
        assert own["status"][0] == 0 and np.isfinite(own["smoothed_covs"]).all()
        for key in KEYS:
            assert_array_equal(out[key][i], own[key][0], err_msg=f"{key}, draw {i}")
