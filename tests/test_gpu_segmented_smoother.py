"""GPU: the smoother across dated structural breaks (dsge_kalman_smoother_segments_batched; csrc/dsge_kalman_seg.hpp,
csrc/dsge_kalman_smooth.hpp, docs/design/segmented_smoother.md) against the numpy reference (tests/segmented_smoother_reference.py:
the chained oracle filter and the pinv recursion) on the cases of tests/segmented_smoother_cases.py, at the project's fixed bars:
states, covariances, shocks and per-step filter moments 1e-9 of each block's scale, ll 1e-8 of max |ll|, status equal.  Then the
device against itself (bits) and against the entries it generalises, and failures that stay local."""
import numpy as np
import pytest

from geconpy_amd import _lib, batched
from geconpy_amd import workloads as wl

from tests import segmented_filter_cases as K
from tests import segmented_smoother_cases as SSC

pytestmark = pytest.mark.gpu

LL_RTOL, RTOL = 1e-8, 1e-9
KEYS = SSC.KEYS
MEANS, COVS = ("a_pred", "a_filt", "smoothed_states"), ("P_pred", "P_filt", "smoothed_covs")


def _run(c, front=batched.kalman_smoother_segments_batched, full_covariances=True, **over):
    a = dict(Hdiag=c["H"], d=c["d"], a0=c["a0"], P0=c["P0"], shift=c["shift"], q_mode=c["q_mode"], full_covariances=full_covariances)
    a.update(over)
    head = [a.pop(key, c[key]) for key in ("T", "R", "q", "Z", "y", "seg_start")]
    return front(*head, **a)


def _err(got, want, scale):
    """Largest difference over the entries the reference defines, by the scale; the NaN patterns must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    diff = np.abs(got - want)
    return 0.0 if np.isnan(diff).all() else float(np.nanmax(diff)) / scale


def _check_draw(res, b, r, scale, label, rows=slice(None), shock_rows=slice(None)):
    sa, sp, se = scale
    errs = {key: _err(res[key][b][rows], r[key][rows], sa) for key in MEANS[:2]}
    errs.update({key: _err(res[key][b][rows], r[key][rows], sp) for key in COVS[:2]})
    errs["ll"] = _err(res["ll"][b], r["ll"], np.abs(r["ll"]).max())
    for key, sc, rw in (("smoothed_states", sa, rows), ("smoothed_covs", sp, rows), ("smoothed_shocks", se, shock_rows)):
        errs[key] = _err(res[key][b][rw], r[key][rw], sc)
    print(f"{label} draw {b}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()) + f" status {res['status'][b]}")
    assert errs.pop("ll") <= LL_RTOL and max(errs.values()) <= RTOL, (label, b, errs)


def _check(res, ref, c, label):
    """The device's outputs of every draw against the reference's, each figure printed before it is held to its bar."""
    for b, r in ref.items():
        assert res["status"][b] == 0
        _check_draw(res, b, r, SSC.scales(c, b, r), label)


@pytest.mark.parametrize("name", SSC.ACCURACY_CASES)
def test_device_equals_reference(name):
    SSC.check_conditions(name)
    c = SSC.case(name)
    res = _run(c)
    _check(res, SSC.reference(name), c, name)
    assert np.isnan(res["smoothed_shocks"][:, 0]).all()
    if c["y"].shape[0] == 1:  # T_len == 1: smoothed = filtered
        assert np.array_equal(res["smoothed_states"], res["a_filt"]) and np.array_equal(res["smoothed_covs"], res["P_filt"])


def test_all_filter_conventions():
    """All 48 combinations on the 17-variable case, under the missing-data rule of tests/test_gpu_conventions.py: the 24 without the
    jitter on F run on the same panel with the missing entry restored (there the filter is not defined in the reference itself)."""
    c, full = SSC.case(K.CONVENTION_CASE), SSC.case(K.CONVENTION_CASE_COMPLETE)
    keep = ~np.isnan(c["y"])
    assert c["T"].shape[2] == 17 and (~keep).sum() == 1 and np.array_equal(c["y"][keep], full["y"][keep]) and len(K.CONVENTIONS) == 48
    for conv in K.CONVENTIONS:
        cc = c if conv["jitter_on_F"] else full
        _check(_run(cc, options=_lib.filter_conventions(**conv)), SSC.reference_of(cc, conv), cc, str(conv))


# ---- the device against itself ------------------------------------------------------------------------------------------------------
def _same_bits(a, b, keys=KEYS + ("status",)):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def _tiled(c, S):
    """A case with one segment repeated S times."""
    rep = lambda x, shared: None if x is None else np.ascontiguousarray(  # noqa: E731
        np.repeat(x, S, axis=0) if x.ndim == shared else np.repeat(x, S, axis=1))
    q_shared = c["q_mode"] in ("diag", "full")
    return dict(c, T=rep(c["T"], -1), R=rep(c["R"], -1), q=np.repeat(c["q"], S, axis=0 if q_shared else 1), Z=rep(c["Z"], 3),
                d=rep(c["d"], 2), H=rep(c["H"], 2))


def _one_draw(c, b):
    """Draw b of a case as a batch of its own."""
    cut = lambda x, shared: x if x is None or x.ndim == shared else x[b:b + 1]  # noqa: E731
    return dict(c, T=c["T"][b:b + 1], R=c["R"][b:b + 1], q=c["q"] if c["q_mode"] in ("diag", "full") else c["q"][b:b + 1],
                Z=cut(c["Z"], 3), d=cut(c["d"], 2), H=cut(c["H"], 2), a0=cut(c["a0"], 0), P0=cut(c["P0"], 0), shift=cut(c["shift"], 0))


def _neighbours_keep_their_bits(c, res, others, **kw):
    for b in others:
        alone = _run(_one_draw(c, b), **kw)
        assert alone["status"][0] == res["status"][b] == 0
        for key in KEYS:
            assert np.array_equal(res[key][b], alone[key][0], equal_nan=True), (key, b)


def test_identical_segments_have_the_bits_of_one_segment():
    one = SSC.case("s1")
    want = _run(one)
    _same_bits(_run(dict(_tiled(one, 3), seg_start=(0, 3, 6))), want)
    _same_bits(_run(dict(_tiled(one, 8), seg_start=tuple(range(8)))), want)


def test_covariance_forms():
    """Diagonals are the diagonals of the full matrices, bit for bit; without the smoothed covariances the covariance recursion is
    skipped and the states and shocks keep their bits."""
    c = SSC.case("ranks_m33")
    full, diag = _run(c), _run(c, full_covariances=False)
    for key in KEYS + ("status",):
        want = np.diagonal(full[key], axis1=2, axis2=3) if key in COVS else full[key]
        assert np.array_equal(diag[key], want, equal_nan=True), key
    lean = _run(c, outputs=("smoothed_states", "smoothed_shocks"))
    _same_bits(lean, full, keys=("smoothed_states", "smoothed_shocks", "status"))
    assert all(lean[key] is None for key in KEYS if key not in ("smoothed_states", "smoothed_shocks"))


def test_every_front_end_subset_and_chunking_has_the_same_bits():
    import torch

    from geconpy_amd.engine import LogpEngine

    c = SSC.case("shift_a0_P0")
    want = _run(c)  # (the host twin)
    _same_bits(_run(c), want)  # a second call
    for key in KEYS:
        one = _run(c, outputs=(key,))
        _same_bits(one, want, keys=(key, "status"))
        assert all(one[other] is None for other in KEYS if other != key)
    nb, S, m, _ = c["T"].shape
    per_draw = batched.segment_smoother_scratch_bytes_per_draw(m, c["y"].shape[0], S)
    _same_bits(_run(c, scratch_limit_bytes=1), want)  # one draw per chunk
    _same_bits(_run(K.build("sw17", nb=3), scratch_limit_bytes=2 * batched.segment_smoother_scratch_bytes_per_draw(17, 8, 3)),
               _run(K.build("sw17", nb=3)))  # chunks of two draws and one
    assert per_draw == 8 * (2 * 8 * m * m + 2 * 8 * m + 3 * S * 48 * 50)
    # a shared Q, repeated per draw once for all chunks, with P0 from the gathered segment 0 of every chunk, the partial last one included
    for q_mode in ("diag", "full"):
        s = K.build("dense5", nb=3, seg_start=(0, 4, 9), n=12, q_mode=q_mode)
        assert s["P0"] is None and s["q"].shape[0] == 3 and s["T"].shape[:3] == (3, 3, 5)
        whole = _run(s)
        assert not whole["status"].any()
        _same_bits(_run(s, scratch_limit_bytes=2 * batched.segment_smoother_scratch_bytes_per_draw(5, 12, 3)), whole)
        like = batched.kalman_logp_segments_batched(s["T"], s["R"], s["q"], s["Z"], s["y"], s["seg_start"], Hdiag=s["H"], d=s["d"],
                                                    q_mode=q_mode)
        assert np.array_equal(whole["ll"], like["ll"]) and np.array_equal(whole["status"], like["status"])
    eng = LogpEngine(0)
    dev = lambda x: None if x is None else eng.to_device(x)  # noqa: E731
    head = [dev(c[key]) for key in ("T", "R", "q", "Z", "y")]
    kw = dict(Hdiag=dev(c["H"]), d=dev(c["d"]), a0=dev(c["a0"]), P0=dev(c["P0"]), shift=dev(c["shift"]), q_mode=c["q_mode"],
              full_covariances=True)
    host = lambda r: {key: r[key].cpu().numpy() for key in KEYS + ("status",)}  # noqa: E731
    res = eng.kalman_smoother_segments(*head, c["seg_start"], **kw)
    torch.cuda.synchronize()
    _same_bits(host(res), want)
    out = {key: torch.full(want[key].shape, 7.0, dtype=torch.float64, device=eng.device) for key in KEYS}
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        res = eng.kalman_smoother_segments(*head, c["seg_start"], out=out, **kw)
    side.synchronize()
    assert all(res[key] is out[key] for key in KEYS)
    _same_bits(host(res), want)


def test_one_segment_agrees_with_the_plain_smoother():
    c = SSC.case("s1")
    res = _run(c)
    out = batched.kalman_smoother_batched(c["T"][:, 0], c["R"][:, 0], c["q"][:, 0], c["Z"][0], c["y"], d=c["d"][0], Hdiag=c["H"][0],
                                          q_mode="diag_batched", full_covariances=True)
    assert not out["status"].any() and not res["status"].any()
    for b, r in SSC.reference("s1").items():
        sa, sp, se = SSC.scales(c, b, r)
        errs = (_err(res["ll"][b], out["ll"][b], np.abs(out["ll"][b]).max()), _err(res["smoothed_states"][b], out["smoothed_states"][b], sa),
                _err(res["smoothed_covs"][b], out["smoothed_covs"][b], sp), _err(res["smoothed_shocks"][b], out["smoothed_shocks"][b], se))
        print(f"draw {b}: ll {errs[0]:.2e} states {errs[1]:.2e} covs {errs[2]:.2e} shocks {errs[3]:.2e}")
        assert errs[0] <= LL_RTOL and max(errs[1:]) <= RTOL
    print("bit-identical to kalman_smoother_batched:", {key: bool(np.array_equal(res[key], out[key], equal_nan=True))
                                                        for key in ("ll", "smoothed_states", "smoothed_covs", "smoothed_shocks")})


def test_forward_outputs_agree_with_the_likelihood_entry():
    c = SSC.case("shift_a0_P0")
    res = _run(c)
    like = batched.kalman_logp_segments_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], c["seg_start"], Hdiag=c["H"], d=c["d"], a0=c["a0"],
                                                P0=c["P0"], shift=c["shift"], q_mode=c["q_mode"])
    e_ll = np.abs(res["ll"] - like["ll"]).max() / np.abs(like["ll"]).max()
    e_lp = np.abs(res["ll"].sum(axis=1) / like["logp"] - 1.0).max()
    e_a = np.abs(res["a_filt"][:, -1] - like["a_last"]).max() / np.abs(like["a_last"]).max()
    e_p = np.abs(res["P_filt"][:, -1] - like["P_last"]).max() / np.abs(like["P_last"]).max()
    print(f"ll {e_ll:.2e} logp {e_lp:.2e} a_last {e_a:.2e} P_last {e_p:.2e}")
    assert not like["status"].any() and not res["status"].any()
    assert e_ll <= LL_RTOL and e_lp <= LL_RTOL and e_a <= RTOL and e_p <= RTOL


# ---- failures stay local ---------------------------------------------------------------------------------------------------------------
def _all_nan(res, b, keys=KEYS):
    return all(np.isnan(res[key][b]).all() for key in keys)


def test_an_incoming_status_skips_the_draw_and_nothing_else():
    c = SSC.case("obs_batched")
    res = _run(c, status=np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32))
    assert list(res["status"]) == [0, _lib.ST_NOT_CONVERGED, 0] and _all_nan(res, 1)
    _neighbours_keep_their_bits(c, res, (0, 2))


def test_a_unit_root_in_segment_zero_fails_like_the_likelihood():
    c = SSC.case("obs_batched")
    T = np.array(c["T"])
    T[1, 0] /= np.abs(np.linalg.eigvals(T[1, 0])).max()
    c = dict(c, T=T)
    res = _run(c)
    like = batched.kalman_logp_segments_batched(T, c["R"], c["q"], c["Z"], c["y"], c["seg_start"], Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"])
    print("status", res["status"], like["status"])
    assert res["status"][1] == like["status"][1] != 0 and res["status"][1] & _lib.ST_LYAP_FAIL and _all_nan(res, 1)
    _neighbours_keep_their_bits(c, res, (0, 2))


def test_a_forward_pass_that_goes_non_finite():
    """Draw 1: the second row of Z is zero and so is its measurement error, so without the F jitter F[1, 1] is exactly 0 in every
    period (finite arithmetic: the factorisation reports it, nothing faults) -- the case of tests/smoother_cases.py, across breaks."""
    c = dict(K.build("sw17", nb=3, missing=()))
    S = c["T"].shape[1]
    Z = np.tile(np.eye(2, 17), (3, S, 1, 1)) * (1.0 + np.arange(S) / 16.0)[None, :, None, None]
    Z[1, :, 1] = 0.0
    c.update(Z=Z, H=np.tile(np.array([K.H0, 0.0]), (S, 1)), d=None, y=np.ascontiguousarray(c["y"][:, :2]))
    kw = dict(options=_lib.filter_conventions(jitter_on_F=False))
    res = _run(c, **kw)
    print("status", res["status"])
    assert list(res["status"]) == [0, _lib.ST_FILTER_NONFINITE, 0] and _all_nan(res, 1, ("smoothed_states", "smoothed_covs", "smoothed_shocks"))
    _neighbours_keep_their_bits(c, res, (0, 2), **kw)
    ref = SSC.reference_of(_one_draw(c, 0), dict(jitter_on_F=False))[0]
    _check_draw(res, 0, ref, SSC.scales(c, 0, ref), "forward_fail")


def test_a_singular_middle_segment_sets_the_status_and_keeps_the_later_steps():
    """Without the P jitter.  Draw 1, segments 0 and 1: the second variable has no shock and no link to the first, so its predicted
    variance and both off-diagonals are exactly 0 and the second pivot of M is exactly 0 (the construction of ``singular_m_nojit``
    in tests/smoother_cases.py); segment 2 couples the two.  Walking back, the steps into periods 7 and 6 are regular, the step into
    period 5 -- the last of the middle segment -- is singular: it and all earlier ones are NaN, the later ones stay."""
    good, bad = np.array([[0.5, 0.0], [0.3, 0.4]]), np.diag([0.5, 0.5])
    T = np.stack([np.stack([good] * 3), np.stack([bad, 0.9 * bad, good]), np.stack([good] * 3)])
    R = np.stack([np.stack([[[1.0], [0.5]]] * 3), np.array([[[1.0], [0.0]], [[1.0], [0.0]], [[1.0], [0.5]]]), np.stack([[[1.0], [0.5]]] * 3)])
    c = dict(T=T, R=R, q=np.array([[1.0], [2.0], [0.5]]), q_mode="diag", Z=np.tile(np.array([[1.0, 0.0]]), (3, 1, 1)), d=None,
             H=np.full((3, 1), 0.01), y=np.random.default_rng(12).standard_normal((8, 1)), seg_start=(0, 3, 6), a0=None, P0=None, shift=None)
    conv = dict(jitter_on_P=False)
    kw = dict(options=_lib.filter_conventions(**conv))
    res = _run(c, **kw)
    print("status", res["status"])
    assert list(res["status"]) == [0, _lib.ST_SMOOTHER_SINGULAR, 0]
    for key in ("smoothed_states", "smoothed_covs"):
        assert np.isnan(res[key][1][:5]).all() and np.isfinite(res[key][1][5:]).all(), key
    assert np.isnan(res["smoothed_shocks"][1][:6]).all() and np.isfinite(res["smoothed_shocks"][1][6:]).all()
    ref = SSC.reference_of(c, conv)
    _check_draw(res, 1, ref[1], SSC.scales(c, 1, ref[1]), "singular middle, later steps", rows=slice(5, None), shock_rows=slice(6, None))
    for b in (0, 2):
        _check_draw(res, b, ref[b], SSC.scales(c, b, ref[b]), "singular middle, neighbours")
    _neighbours_keep_their_bits(c, res, (0, 2), **kw)


def test_fused_front_end_against_the_reference():
    nb, S = 3, 3
    b = wl.sw_shaped_batch(nb, **dict(zip(("n", "n_state", "n_lead", "k"), K.SC.SW17)))
    pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % nb
    c = K.build("sw17", nb=nb)
    assert np.array_equal(c["T"], b["T_star"][pick])  # (the case is built from the same systems)
    sys_ = [np.ascontiguousarray(b[x][pick]) for x in "ABCD"]
    kw = dict(Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], full_covariances=True)
    res = batched.solve_kalman_smoother_segments_batched(*sys_, c["q"], c["Z"], c["y"], c["seg_start"], tol=1e-9, max_iter=1000, **kw)
    assert np.abs(res["T"] - c["T"]).max() <= 1e-9 and np.abs(res["R"] - c["R"]).max() <= 1e-8  # (the bars of the solver entries)
    _check(res, SSC.reference_of(c), c, "fused")
    # gensys: the same plumbing behind another solver entry, held to the reference on the T and R it returned
    other = batched.solve_kalman_smoother_segments_batched(*sys_, c["q"], c["Z"], c["y"], c["seg_start"], solver="gensys", tol=1e-8, **kw)
    cc = dict(c, T=other["T"], R=other["R"])
    _check(other, SSC.reference_of(cc), cc, "gensys")


def test_sizes_beyond_the_entry_are_refused_and_empty_calls_touch_nothing():
    c = SSC.case("s1")
    lib = _lib.load()
    ptr = lambda x: x.ctypes.data  # noqa: E731
    T, R, q, Z, seg = np.zeros((1, 1, 65, 65)), np.zeros((1, 1, 65, 1)), np.ones((1, 1)), np.zeros((1, 4, 65)), np.zeros(1, dtype=np.int32)
    out, st = np.zeros((1, 8, 65)), np.zeros(1, dtype=np.int32)
    assert lib.dsge_kalman_smoother_segments_batched_host(ptr(T), ptr(R), ptr(q), 0, ptr(Z), 0, None, 0, None, 0, None, None, None,
                                                          ptr(np.ascontiguousarray(c["y"])), ptr(seg), 1, 1, 65, 1, 4, 8, 1e-8, -9999.0, 0.0, 0,
                                                          0, None, None, None, None, None, ptr(out), None, None, ptr(st)) == _lib.ERR_TOO_LARGE
    r = batched.kalman_smoother_segments_batched(c["T"][:0], c["R"][:0], c["q"][:0], c["Z"], c["y"], (0,), q_mode="diag_batched")
    assert r["smoothed_states"].shape == (0, 8, 17)
    r = batched.kalman_smoother_segments_batched(c["T"], c["R"], c["q"], c["Z"], c["y"][:0], (0,), q_mode="diag_batched")
    assert r["smoothed_states"].shape == (c["T"].shape[0], 0, 17)
