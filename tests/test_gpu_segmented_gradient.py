"""GPU: the gradient of the Kalman likelihood across dated structural breaks (dsge_kalman_logp_segments_grad_batched;
csrc/dsge_kalman_seg_grad.hpp, docs/design/segmented_gradient.md) against the float64 autograd reference
(tests/segmented_gradient_reference.py) on the cases of tests/segmented_filter_cases.py and that module's own (``GRADIENT_CASES``): EVERY entry of every block held to 1e-9 of
the block's largest reference entry (the project's bar for adjoints, tests/test_gpu_gradient_entries.py), logp to 1e-8 relative, status
equal.  A block whose reference is identically zero (tests/test_segmented_gradient_reference.py says which may be) must be exactly zero
on the device.  Then the device against itself (bits), and failures that stay local.

A case x block listed in ROUNDING takes 1e-8, with its cause and the measured figure (docs/design/segmented_gradient.md names them)."""
import numpy as np
import pytest

from geconpy_amd import _lib, batched
from geconpy_amd import workloads as wl

from tests import segmented_filter_cases as K
from tests import segmented_gradient_reference as G

pytestmark = pytest.mark.gpu

BAR, GENSYS_BAR, LOGP_RTOL = 1e-9, 1e-7, 1e-8
ROUNDING_BAR = 1e-8
ROUNDING = {}  # (case, block) -> (cause, measured): rounding of a documented algorithm, held to ROUNDING_BAR
BLOCKS = ("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar", "a0_bar", "P0_bar")


def _qkey(c):
    return "Q_bar" if c["q_mode"] in ("full", "full_batched") else "q_bar"


def _keys(c):
    return tuple(_qkey(c) if key == "q_bar" else key for key in BLOCKS)


def _run(c, front=batched.kalman_logp_segments_grad_batched, **over):
    a = dict(Hdiag=c["H"], d=c["d"], a0=c["a0"], P0=c["P0"], shift=c["shift"], q_mode=c["q_mode"])
    a.update(over)
    head = [a.pop(key, c[key]) for key in ("T", "R", "q", "Z", "y", "seg_start")]
    return front(*head, **a)


def _check(res, ref, c, label, bar=BAR, keys=None):
    """Every block of every draw against the reference's, each figure printed before it is held to its bar.  Returns the worst
    error per block."""
    worst = {}
    for b, r in ref.items():
        e_lp = abs(res["logp"][b] - r["logp"]) / abs(r["logp"])
        line = [f"logp {e_lp:.2e}"]
        missed = []
        for key in keys or _keys(c):
            got, want = res[key][b], r[key]
            assert got.shape == want.shape, (label, key, got.shape, want.shape)
            assert np.isfinite(got).all(), (label, b, key)
            scale = np.abs(want).max()
            if scale == 0.0:
                assert not got.any(), (label, b, key, "the reference block is zero")
                continue
            err = np.abs(got - want).max() / scale
            worst[key] = max(worst.get(key, 0.0), err)
            line.append(f"{key} {err:.2e}")
            if not err <= (ROUNDING_BAR if (label, key) in ROUNDING else bar):
                missed.append((key, err))
        print(f"{label} draw {b}: " + " ".join(line) + f" status {res['status'][b]}")
        assert res["status"][b] == 0, (label, b)
        assert e_lp <= LOGP_RTOL, (label, b, e_lp)
        assert not missed, (label, b, missed)
    return worst


@pytest.mark.parametrize("name", G.GRADIENT_CASES)
def test_every_entry_of_the_gradient(name):
    c = G.case(name)
    res = _run(c)
    _check(res, G.case_reference(name), c, name)
    if c["P0"] is not None:  # the Lyapunov adjoint did not run: T_bar of segment 0 is the sweep's alone (the reference's, held above)
        assert all(np.abs(res["P0_bar"][b]).max() > 0.0 and np.abs(r["P0_bar"]).max() > 0.0 for b, r in G.case_reference(name).items())
    lp = batched.kalman_logp_segments_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], c["seg_start"], Hdiag=c["H"], d=c["d"], a0=c["a0"],
                                              P0=c["P0"], shift=c["shift"], q_mode=c["q_mode"], outputs=("logp",))
    assert np.array_equal(res["logp"], lp["logp"]) and np.array_equal(res["status"], lp["status"])


def test_all_filter_conventions():
    """All 48 combinations on the 17-variable case; the 24 without the jitter on F on the panel with its missing entry restored
    (the rule of tests/test_gpu_conventions.py: under missing data that filter is not defined in the reference itself)."""
    c, full = K.case(K.CONVENTION_CASE), K.case(K.CONVENTION_CASE_COMPLETE)
    assert c["T"].shape[2] == 17 and len(K.CONVENTIONS) == 48
    worst = {}
    for conv in K.CONVENTIONS:
        cc = c if conv["jitter_on_F"] else full
        w = _check(_run(cc, options=_lib.filter_conventions(**conv)), G.reference(cc, conv), cc, str(conv))
        worst = {key: max(worst.get(key, 0.0), err) for key, err in w.items()}
    print("conventions, worst:", " ".join(f"{key} {err:.2e}" for key, err in worst.items()))


# ---- the fused front end ---------------------------------------------------------------------------------------------------------------
def _fused_inputs(nb=3, S=3):
    sh = dict(zip(("n", "n_state", "n_lead", "k"), K.SC.SW17))
    b = wl.sw_shaped_batch(nb, **sh)
    pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % nb
    c = K.build("sw17", nb=nb)
    assert np.array_equal(c["T"], b["T_star"][pick])  # (the case is built from the same systems)
    return c, {x: np.ascontiguousarray(b[x][pick]) for x in "ABCD"}


@pytest.fixture(scope="module")
def fused_reference():
    c, sys_ = _fused_inputs()
    return {b: G.fused_logp_and_gradient(sys_["A"][b], sys_["B"][b], sys_["C"][b], sys_["D"][b], c, b) for b in range(c["T"].shape[0])}


@pytest.mark.parametrize("solver,bar,kw", [("cycle_reduction", BAR, dict(tol=1e-13, max_iter=1000)), ("gensys", GENSYS_BAR, dict(tol=1e-8))])
def test_fused_front_end_against_the_reference(solver, bar, kw, fused_reference):
    c, sys_ = _fused_inputs()
    res = batched.solve_kalman_logp_segments_grad_batched(sys_["A"], sys_["B"], sys_["C"], sys_["D"], c["q"], c["Z"], c["y"], c["seg_start"],
                                                          Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], solver=solver, **kw)
    _check(res, fused_reference, c, solver, bar=bar, keys=("A_bar", "B_bar", "C_bar", "D_bar") + _keys(c))


def test_fused_front_end_keeps_a_singular_segment_local():
    c, sys_ = _fused_inputs()
    kw = dict(Hdiag=c["H"], d=c["d"], q_mode=c["q_mode"], tol=1e-13, max_iter=1000)
    tail = (c["q"], c["Z"], c["y"], c["seg_start"])
    want = batched.solve_kalman_logp_segments_grad_batched(*(sys_[x] for x in "ABCD"), *tail, **kw)
    bad = {x: v.copy() for x, v in sys_.items()}
    bad["B"][1, 2] = 0.0  # segment 2 of draw 1: B + C T = 0 for every T the iteration reaches from a zero B and C
    bad["C"][1, 2] = 0.0
    res = batched.solve_kalman_logp_segments_grad_batched(*(bad[x] for x in "ABCD"), *tail, **kw)
    keys = ("A_bar", "B_bar", "C_bar", "D_bar") + _keys(c)
    print("status", res["status"])
    assert res["status"][1] != 0 and res["logp"][1] == -np.inf and not res["status"][[0, 2]].any()
    for key in keys:
        assert not res[key][1].any(), key
        assert np.array_equal(res[key][[0, 2]], want[key][[0, 2]]), key
    assert np.array_equal(res["logp"][[0, 2]], want["logp"][[0, 2]])
    import torch

    from geconpy_amd.engine import LogpEngine

    eng = LogpEngine(0)
    dev = eng.to_device
    got = eng.solve_kalman_logp_segments_grad(*(dev(bad[x]) for x in "ABCD"), dev(c["q"]), dev(c["Z"]), dev(c["y"]), c["seg_start"],
                                              Hdiag=dev(c["H"]), d=dev(c["d"]), q_mode=c["q_mode"], tol=1e-13, max_iter=1000)
    torch.cuda.synchronize()
    for key in keys + ("logp", "status"):
        assert np.array_equal(got[key].cpu().numpy(), res[key]), key


# ---- the device against itself ------------------------------------------------------------------------------------------------------
def _same_bits(a, b, keys):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def test_every_front_end_every_subset_and_every_chunking_has_the_same_bits():
    import torch

    from geconpy_amd.engine import LogpEngine

    c = K.build("dense33", nb=3, shift=True, a0=True, P0=True)
    keys = _keys(c)
    every = keys + ("logp", "status")
    want = _run(c)
    _same_bits(_run(c), want, every)  # a second call
    for key in keys:
        one = _run(c, outputs=(key,))
        _same_bits(one, want, (key, "logp", "status"))
        assert all(one[other] is None for other in keys if other != key)
    per = batched.segment_gradient_scratch_bytes_per_draw(33, c["y"].shape[0], 3)
    assert per == 8 * (2 * 8 * 33 * 33 + 2 * 8 * 33 + 2 * 3 * 33 * 33)
    _same_bits(_run(c, scratch_limit_bytes=1), want, every)        # one draw per chunk
    _same_bits(_run(c, scratch_limit_bytes=2 * per), want, every)  # chunks of two draws and one
    nop0 = dict(c, P0=None)  # (the Lyapunov adjoint, chunked)
    _same_bits(_run(nop0, scratch_limit_bytes=2 * per), _run(nop0), every)
    # a shared Q, repeated per draw once for all chunks, with P0 from the gathered segment 0 of every chunk, the partial last one included
    for q_mode in ("diag", "full"):
        s = K.build("dense5", nb=3, seg_start=(0, 4, 9), n=12, q_mode=q_mode)
        assert s["P0"] is None and s["q"].shape[0] == 3 and s["T"].shape[:3] == (3, 3, 5)
        whole = _run(s)
        assert not whole["status"].any()
        _same_bits(_run(s, scratch_limit_bytes=2 * batched.segment_gradient_scratch_bytes_per_draw(5, 12, 3)), whole,
                   _keys(s) + ("logp", "status"))
        like = batched.kalman_logp_segments_batched(s["T"], s["R"], s["q"], s["Z"], s["y"], s["seg_start"], Hdiag=s["H"], d=s["d"],
                                                    q_mode=q_mode, outputs=("logp",))
        assert np.array_equal(whole["logp"], like["logp"]) and np.array_equal(whole["status"], like["status"])
    eng = LogpEngine(0)
    dev = lambda x: None if x is None else eng.to_device(x)  # noqa: E731
    head = [dev(c[key]) for key in ("T", "R", "q", "Z", "y")]
    kw = dict(Hdiag=dev(c["H"]), d=dev(c["d"]), a0=dev(c["a0"]), P0=dev(c["P0"]), shift=dev(c["shift"]), q_mode=c["q_mode"])
    host = lambda r: {key: r[key].cpu().numpy() for key in every}  # noqa: E731
    res = eng.kalman_logp_segments_grad(*head, c["seg_start"], **kw)
    torch.cuda.synchronize()
    _same_bits(host(res), want, every)
    out = {key: torch.full(want[key].shape, 7.0, dtype=torch.float64, device=eng.device) for key in keys + ("logp",)}
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        res = eng.kalman_logp_segments_grad(*head, c["seg_start"], out=out, **kw)
    side.synchronize()
    assert all(res[key] is out[key] for key in keys + ("logp",))
    _same_bits(host(res), want, every)


def _tiled(c, S):
    """A case with one segment repeated S times."""
    rep = lambda x, shared: None if x is None else np.ascontiguousarray(  # noqa: E731
        np.repeat(x, S, axis=0) if x.ndim == shared else np.repeat(x, S, axis=1))
    q_shared = c["q_mode"] in ("diag", "full")
    return dict(c, T=rep(c["T"], -1), R=rep(c["R"], -1), q=np.repeat(c["q"], S, axis=0 if q_shared else 1), Z=rep(c["Z"], 3),
                d=rep(c["d"], 2), H=rep(c["H"], 2))


def test_identical_segments_sum_to_one_segment():
    """S = 3 with identical matrices and no shift: each cotangent summed over its segments is the S = 1 call's, to 1e-12 of scale (not
    bitwise: the order of summation differs)."""
    one = K.case("s1")
    want, got = _run(one), _run(dict(_tiled(one, 3), seg_start=(0, 3, 6)))
    assert np.array_equal(want["logp"], got["logp"])
    for key in ("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar"):
        err = np.abs(got[key].sum(axis=1) - want[key][:, 0]).max() / np.abs(want[key]).max()
        print(f"{key} {err:.2e}")
        assert err <= 1e-12, key
    assert np.array_equal(got["a0_bar"], want["a0_bar"])


# ---- failures stay local ---------------------------------------------------------------------------------------------------------------
def _failed_draw_is_zero_and_neighbours_keep_their_bits(c, res, want, bad):
    keys = _keys(c)
    good = [b for b in range(c["T"].shape[0]) if b != bad]
    assert res["logp"][bad] == -np.inf
    for key in keys:
        assert not res[key][bad].any(), key
        assert np.array_equal(res[key][good], want[key][good]), key
    assert np.array_equal(res["logp"][good], want["logp"][good]) and not res["status"][good].any()


def test_an_incoming_status_skips_the_draw_and_nothing_else():
    c = K.case("obs_batched")
    res = _run(c, status=np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32))
    assert list(res["status"]) == [0, _lib.ST_NOT_CONVERGED, 0]
    _failed_draw_is_zero_and_neighbours_keep_their_bits(c, res, _run(c), 1)


def test_a_unit_root_in_segment_zero():
    c = K.case("obs_batched")
    T = np.array(c["T"])
    T[1, 0] /= np.abs(np.linalg.eigvals(T[1, 0])).max()
    res = _run(c, T=T)
    print("status", res["status"])
    assert res["status"][1] & _lib.ST_LYAP_FAIL
    _failed_draw_is_zero_and_neighbours_keep_their_bits(c, res, _run(c), 1)


def test_a_forward_pass_that_goes_non_finite():
    """Draw 1: the second row of Z is zero and so is its measurement error, so without the F jitter F[1, 1] is exactly 0 in every
    period (finite arithmetic: the factorisation reports it, nothing faults) -- the case of tests/test_gpu_segmented_smoother.py."""
    c = dict(K.build("sw17", nb=3, missing=()))
    S = c["T"].shape[1]
    Z = np.tile(np.eye(2, 17), (3, S, 1, 1)) * (1.0 + np.arange(S) / 16.0)[None, :, None, None]
    good = Z.copy()
    Z[1, :, 1] = 0.0
    c.update(H=np.tile(np.array([K.H0, 0.0]), (S, 1)), d=None, y=np.ascontiguousarray(c["y"][:, :2]))
    kw = dict(options=_lib.filter_conventions(jitter_on_F=False))
    res = _run(dict(c, Z=Z), **kw)
    print("status", res["status"])
    assert list(res["status"]) == [0, _lib.ST_FILTER_NONFINITE, 0]
    _failed_draw_is_zero_and_neighbours_keep_their_bits(c, res, _run(dict(c, Z=good), **kw), 1)


def test_sizes_beyond_the_entry_are_refused():
    c = K.case("s1")
    with pytest.raises(ValueError):
        batched.kalman_logp_segments_grad_batched(np.zeros((1, 1, 65, 65)), np.zeros((1, 1, 65, 1)), np.ones((1, 1)), np.zeros((1, 4, 65)),
                                                  c["y"], (0,))
    r = batched.kalman_logp_segments_grad_batched(c["T"][:0], c["R"][:0], c["q"][:0], c["Z"], c["y"], (0,), q_mode="diag_batched")
    assert r["logp"].shape == (0,) and r["T_bar"].shape == (0, 1, 17, 17)
