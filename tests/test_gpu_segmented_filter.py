"""GPU: the Kalman likelihood across dated structural breaks (dsge_kalman_logp_segments_batched; csrc/dsge_kalman_seg.hpp,
docs/design/segmented_filter.md) against the numpy reference (tests/segmented_filter_reference.py: oracle.kalman_filter_logp chained
segment by segment) on the cases of tests/segmented_filter_cases.py, at the project's fixed bars: logp 1e-8 relative, ll 1e-8 of
max |ll|, a_last and P_last 1e-9 of their largest entry, status equal.  Then the device against itself (bits), and failures that
stay local."""
import numpy as np
import pytest

from geconpy_amd import _lib, batched
from geconpy_amd import workloads as wl

from tests import segmented_filter_cases as K

pytestmark = pytest.mark.gpu

LOGP_RTOL, LL_RTOL, STATE_RTOL = 1e-8, 1e-8, 1e-9
OUTPUTS = ("logp", "ll", "a_last", "P_last")


def _run(c, front=batched.kalman_logp_segments_batched, **over):
    a = dict(Hdiag=c["H"], d=c["d"], a0=c["a0"], P0=c["P0"], shift=c["shift"], q_mode=c["q_mode"])
    a.update(over)
    head = [a.pop(key, c[key]) for key in ("T", "R", "q", "Z", "y", "seg_start")]
    return front(*head, **a)


def _check(res, ref, label):
    """The device's outputs of every draw against the reference's, each figure printed before it is held to its bar."""
    for b, r in ref.items():
        e_lp = abs(res["logp"][b] - r["logp"]) / abs(r["logp"])
        e_ll = np.abs(res["ll"][b] - r["ll"]).max() / np.abs(r["ll"]).max()
        e_a = np.abs(res["a_last"][b] - r["a_last"]).max() / np.abs(r["a_last"]).max()
        e_p = np.abs(res["P_last"][b] - r["P_last"]).max() / np.abs(r["P_last"]).max()
        print(f"{label} draw {b}: logp {e_lp:.2e} ll {e_ll:.2e} a_last {e_a:.2e} P_last {e_p:.2e} status {res['status'][b]}")
        assert res["status"][b] == 0
        assert e_lp <= LOGP_RTOL and e_ll <= LL_RTOL and e_a <= STATE_RTOL and e_p <= STATE_RTOL, (label, b)


@pytest.mark.parametrize("name", K.ACCURACY_CASES)
def test_device_equals_reference(name):
    K.check_conditions(name)
    _check(_run(K.case(name)), K.reference(name), name)


def test_all_filter_conventions():
    """All 48 combinations on the 17-variable case.  With the jitter on F the panel has its missing entry; without it the filter is
    not defined under missing data in the reference itself (the masked row of Z and H is zero: F is singular and the oracle raises),
    so those 24 run on the same panel with the entry restored -- the rule of tests/test_gpu_conventions.py."""
    c, full = K.case(K.CONVENTION_CASE), K.case(K.CONVENTION_CASE_COMPLETE)
    keep = ~np.isnan(c["y"])
    assert c["T"].shape[2] == 17 and (~keep).sum() == 1 and np.array_equal(c["y"][keep], full["y"][keep]) and len(K.CONVENTIONS) == 48
    for conv in K.CONVENTIONS:
        cc = c if conv["jitter_on_F"] else full
        _check(_run(cc, options=_lib.filter_conventions(**conv)), K.reference_of(cc, conv), str(conv))


# ---- the device against itself ------------------------------------------------------------------------------------------------------
def _same_bits(a, b, keys=OUTPUTS + ("status",)):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def _one_segment(c, s=0):
    """Segment s of a case as a case of its own (S = 1)."""
    pick = lambda x, shared: None if x is None else (x[s:s + 1] if x.ndim == shared else x[:, s:s + 1])  # noqa: E731
    q_shared = c["q_mode"] in ("diag", "full")
    return dict(c, T=c["T"][:, s:s + 1], R=c["R"][:, s:s + 1], q=c["q"][s:s + 1] if q_shared else c["q"][:, s:s + 1],
                Z=pick(c["Z"], 3), d=pick(c["d"], 2), H=pick(c["H"], 2), seg_start=(0,), shift=None)


def _tiled(c, S):
    """A case with one segment repeated S times."""
    rep = lambda x, shared: None if x is None else np.ascontiguousarray(  # noqa: E731
        np.repeat(x, S, axis=0) if x.ndim == shared else np.repeat(x, S, axis=1))
    q_shared = c["q_mode"] in ("diag", "full")
    return dict(c, T=rep(c["T"], -1), R=rep(c["R"], -1), q=np.repeat(c["q"], S, axis=0 if q_shared else 1), Z=rep(c["Z"], 3),
                d=rep(c["d"], 2), H=rep(c["H"], 2))


def test_identical_segments_have_the_bits_of_one_segment():
    one = K.case("s1")
    want = _run(one)
    _same_bits(_run(dict(_tiled(one, 3), seg_start=(0, 3, 6))), want)
    _same_bits(_run(dict(_tiled(one, 8), seg_start=tuple(range(8)))), want)


def test_one_segment_agrees_with_the_other_filter_entries():
    c = K.case("s1")
    res = _run(c)
    kw = dict(d=c["d"][0], Hdiag=c["H"][0], q_mode="diag_batched")
    out = batched.kalman_filter_outputs_batched(c["T"][:, 0], c["R"][:, 0], c["q"][:, 0], c["Z"][0], c["y"], full_covariances=True, **kw)
    logp, st = batched.kalman_logp_batched(c["T"][:, 0], c["R"][:, 0], c["q"][:, 0], c["Z"][0], c["y"], **kw)
    e_ll = np.abs(res["ll"] - out["ll"]).max() / np.abs(out["ll"]).max()
    e_lp = np.abs(res["logp"] / logp - 1.0).max()
    e_a = np.abs(res["a_last"] - out["filtered_states"][:, -1]).max() / np.abs(out["filtered_states"][:, -1]).max()
    e_p = np.abs(res["P_last"] - out["filtered_covs"][:, -1]).max() / np.abs(out["filtered_covs"][:, -1]).max()
    print(f"ll {e_ll:.2e} logp {e_lp:.2e} a_last {e_a:.2e} P_last {e_p:.2e}")
    assert not st.any() and not out["status"].any() and not res["status"].any()
    assert e_ll <= LL_RTOL and e_lp <= LOGP_RTOL and e_a <= STATE_RTOL and e_p <= STATE_RTOL


def test_chaining_across_entries_reproduces_two_segments():
    tau = 3
    c = K.build("sw17", seg_start=(0, tau), shift=True)
    full = _run(c)
    head = _run(dict(_one_segment(c, 0), y=c["y"][:tau]))
    fc = batched.forecast_batched(c["T"][:, 1], c["R"][:, 1], c["q"][:, 1], head["a_last"] + c["shift"][:, 1], P0=head["P_last"],
                                  n_steps=1, q_mode="diag_batched", covariances="full")
    tail = _run(dict(_one_segment(c, 1), y=c["y"][tau:], a0=np.ascontiguousarray(fc["states"][:, 0]),
                     P0=np.ascontiguousarray(fc["covs"][:, 0])))
    ll = np.concatenate([head["ll"], tail["ll"]], axis=1)
    e_lp = np.abs((head["logp"] + tail["logp"]) / full["logp"] - 1.0).max()
    e_ll = np.abs(ll - full["ll"]).max() / np.abs(full["ll"]).max()
    e_a = np.abs(tail["a_last"] - full["a_last"]).max() / np.abs(full["a_last"]).max()
    e_p = np.abs(tail["P_last"] - full["P_last"]).max() / np.abs(full["P_last"]).max()
    print(f"logp {e_lp:.2e} ll {e_ll:.2e} a_last {e_a:.2e} P_last {e_p:.2e}")
    assert not full["status"].any() and not head["status"].any() and not tail["status"].any()
    assert e_lp <= LOGP_RTOL and e_ll <= LL_RTOL and e_a <= STATE_RTOL and e_p <= STATE_RTOL


def test_every_front_end_and_every_subset_of_outputs_has_the_same_bits():
    import torch

    from geconpy_amd.engine import LogpEngine

    c = K.case("shift_a0_P0")
    want = _run(c)
    _same_bits(_run(c), want)  # a second call
    for key in OUTPUTS:
        one = _run(c, outputs=(key,))
        _same_bits(one, want, keys=tuple({key, "logp", "status"}))
        assert all(one[other] is None for other in OUTPUTS if other not in (key, "logp"))
    eng = LogpEngine(0)
    dev = lambda x: None if x is None else eng.to_device(x)  # noqa: E731
    head = [dev(c[key]) for key in ("T", "R", "q", "Z", "y")]
    kw = dict(Hdiag=dev(c["H"]), d=dev(c["d"]), a0=dev(c["a0"]), P0=dev(c["P0"]), shift=dev(c["shift"]), q_mode=c["q_mode"])
    host = lambda r: {key: r[key].cpu().numpy() for key in OUTPUTS + ("status",)}  # noqa: E731
    res = eng.kalman_logp_segments(*head, c["seg_start"], **kw)
    torch.cuda.synchronize()
    _same_bits(host(res), want)
    nb, _, m, _ = c["T"].shape
    out = dict(logp=torch.full((nb,), 7.0, dtype=torch.float64, device=eng.device),
               ll=torch.full((nb, c["y"].shape[0]), 7.0, dtype=torch.float64, device=eng.device),
               a_last=torch.full((nb, m), 7.0, dtype=torch.float64, device=eng.device),
               P_last=torch.full((nb, m, m), 7.0, dtype=torch.float64, device=eng.device))
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        res = eng.kalman_logp_segments(*head, c["seg_start"], out=out, **kw)
    side.synchronize()
    assert all(res[key] is out[key] for key in OUTPUTS)
    _same_bits(host(res), want)


# ---- failures stay local ---------------------------------------------------------------------------------------------------------------
def test_an_incoming_status_skips_the_draw_and_nothing_else():
    c = K.case("obs_batched")
    want = _run(c)
    res = _run(c, status=np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32))
    assert list(res["status"]) == [0, _lib.ST_NOT_CONVERGED, 0]
    assert res["logp"][1] == -np.inf
    assert np.isnan(res["ll"][1]).all() and np.isnan(res["a_last"][1]).all() and np.isnan(res["P_last"][1]).all()
    for key in OUTPUTS:
        assert np.array_equal(res[key][[0, 2]], want[key][[0, 2]]), key


def test_a_unit_root_in_segment_zero_fails_like_the_plain_filter():
    c = K.case("obs_batched")
    T = np.array(c["T"])
    T[1, 0] /= np.abs(np.linalg.eigvals(T[1, 0])).max()
    want, res = _run(c), _run(c, T=T)
    logp, st = batched.kalman_logp_batched(T[:, 0], c["R"][:, 0], c["q"][:, 0], c["Z"][:, 0], c["y"], d=c["d"][:, 0], Hdiag=c["H"][:, 0],
                                           q_mode="full_batched" if c["q_mode"].startswith("full") else "diag_batched")
    print("status", res["status"], st, "logp", res["logp"], logp)
    assert res["status"][1] == st[1] != 0 and res["status"][1] & _lib.ST_LYAP_FAIL
    assert res["logp"][1] == logp[1] == -np.inf
    assert np.isnan(res["ll"][1]).all() and np.isnan(res["a_last"][1]).all() and np.isnan(res["P_last"][1]).all()
    for key in OUTPUTS + ("status",):
        assert np.array_equal(res[key][[0, 2]], want[key][[0, 2]]), key


def _fused_inputs(nb=3, S=3):
    sh = dict(zip(("n", "n_state", "n_lead", "k"), K.SC.SW17))
    b = wl.sw_shaped_batch(nb, **sh)
    pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % nb
    c = K.build("sw17", nb=nb)
    assert np.array_equal(c["T"], b["T_star"][pick])  # (the case is built from the same systems)
    return c, {x: np.ascontiguousarray(b[x][pick]) for x in "ABCD"}, b["T_star"][pick]


def test_fused_front_end_against_the_reference():
    c, sys_, T_star = _fused_inputs()
    res = batched.solve_kalman_logp_segments_batched(sys_["A"], sys_["B"], sys_["C"], sys_["D"], c["q"], c["Z"], c["y"], c["seg_start"],
                                                     Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], tol=1e-9, max_iter=1000)
    e_T = np.abs(res["T"] - T_star).max()
    e_R = np.abs(res["R"] - c["R"]).max()
    print(f"T {e_T:.2e} R {e_R:.2e}")
    assert e_T <= 1e-9 and e_R <= 1e-8  # (the bars of tests/test_gpu_parity.py for the solver entries)
    _check(res, K.reference_of(c), "fused")
    # gensys: the same plumbing behind another solver entry, held to the reference on the T and R it returned
    other = batched.solve_kalman_logp_segments_batched(sys_["A"], sys_["B"], sys_["C"], sys_["D"], c["q"], c["Z"], c["y"], c["seg_start"],
                                                       Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], solver="gensys", tol=1e-8)
    print(f"gensys T {np.abs(other['T'] - T_star).max():.2e}")
    _check(other, K.reference_of(dict(c, T=other["T"], R=other["R"])), "gensys")


def test_fused_front_end_keeps_a_singular_segment_local():
    c, sys_, _ = _fused_inputs()
    kw = dict(Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], tol=1e-9, max_iter=1000)
    want = batched.solve_kalman_logp_segments_batched(sys_["A"], sys_["B"], sys_["C"], sys_["D"], c["q"], c["Z"], c["y"], c["seg_start"], **kw)
    bad = {x: v.copy() for x, v in sys_.items()}
    bad["B"][1, 2] = 0.0  # segment 2 of draw 1: B + C T = 0 for every T the iteration reaches from a zero B and C
    bad["C"][1, 2] = 0.0
    res = batched.solve_kalman_logp_segments_batched(bad["A"], bad["B"], bad["C"], bad["D"], c["q"], c["Z"], c["y"], c["seg_start"], **kw)
    nb, S, n, _ = bad["A"].shape
    _, st, _ = batched.cycle_reduction_batched(*(bad[x].reshape(nb * S, n, n) for x in "ABC"), max_iter=1000, tol=1e-9)
    st = st.reshape(nb, S)
    print("solver status", st, "status", res["status"])
    assert st[1, 2] != 0 and not np.delete(st.reshape(-1), 1 * S + 2).any()
    assert res["status"][1] == np.bitwise_or.reduce(st[1]) and res["logp"][1] == -np.inf
    assert np.isnan(res["ll"][1]).all() and np.isnan(res["a_last"][1]).all() and np.isnan(res["P_last"][1]).all()
    for key in OUTPUTS + ("status",):
        assert np.array_equal(res[key][[0, 2]], want[key][[0, 2]]), key
    # the engine's fused front end (device tensors, the status words ORed by torch): the bits of the host front end
    import torch

    from geconpy_amd.engine import LogpEngine

    eng = LogpEngine(0)
    dev = eng.to_device
    got = eng.solve_kalman_logp_segments(*(dev(bad[x]) for x in "ABCD"), dev(c["q"]), dev(c["Z"]), dev(c["y"]), c["seg_start"],
                                         Hdiag=dev(c["H"]), d=dev(c["d"]), q_mode=c["q_mode"], tol=1e-9, max_iter=1000)
    torch.cuda.synchronize()
    _same_bits({key: got[key].cpu().numpy() for key in OUTPUTS + ("status",)}, res)
    assert np.array_equal(got["T"].cpu().numpy()[[0, 2]], res["T"][[0, 2]]) and got["T"].shape == (nb, S, n, n)


def test_sizes_beyond_the_entry_are_refused():
    c = K.case("s1")
    T = np.zeros((1, 1, 65, 65))
    with pytest.raises(_lib.DsgeTooLargeError):
        batched.kalman_logp_segments_batched(T, np.zeros((1, 1, 65, 1)), np.ones((1, 1)), np.zeros((1, 4, 65)), c["y"], (0,))
    # batch == 0 and T_len == 0: success, nothing touched
    r = batched.kalman_logp_segments_batched(c["T"][:0], c["R"][:0], c["q"][:0], c["Z"], c["y"], (0,), q_mode="diag_batched")
    assert r["logp"].shape == (0,)
    lp = batched.kalman_logp_segments_batched(c["T"], c["R"], c["q"], c["Z"], c["y"][:0], (0,), q_mode="diag_batched")
    assert lp["ll"].shape == (c["T"].shape[0], 0)
