"""CPU: the numpy references of the smoother across dated structural breaks (tests/segmented_smoother_reference.py) against each
other -- the pinv recursion against brute-force conditioning of the time-varying system, the range form (the device's) against the
pinv form on the inputs of EVERY device accuracy case, identical segments against ``rts_smoother``, the transition identity across
boundaries -- and the front end against a stand-in library: refusals, layouts, the call sequence of the fused front end, and no
scratch memory in the new kernel instantiations (docs/design/segmented_smoother.md)."""
import os
import re

import numpy as np
import pytest

import oracle
from geconpy_amd import _lib, batched

from tests import segmented_filter_cases as K
from tests import segmented_smoother_cases as SSC
from tests.segmented_filter_reference import segment_of
from tests.segmented_smoother_reference import (brute_force_segmented_smoother, segmented_forward, segmented_range_smoother,
                                                segmented_rts_smoother)
from tests.smoother_reference import rts_smoother

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references against each other -----------------------------------------------------------------------------------------------
def _smooth(c, b, conv=None, form=segmented_rts_smoother):
    cv = None if conv is None else oracle.FilterConventions(**conv)
    segs = K.draw(c, b)
    fwd = segmented_forward(c["y"], segs, c["seg_start"], a0=None if c["a0"] is None else c["a0"][b],
                            P0=None if c["P0"] is None else c["P0"][b], shift=None if c["shift"] is None else c["shift"][b], conventions=cv)
    return segs, fwd, form(fwd, segs, c["seg_start"])


def test_pinv_recursion_matches_joint_gaussian_conditioning():
    """Three segments with breaks at t = 1 and t = 5, a shift, a given a0 / P0, one missing entry in a boundary period (t = 5) and
    one empty period (t = 3); the filter without the P jitter and the Joseph form, so that the stored filter IS the exact filter of
    the time-varying model with noise H_s + jitter_F I.  The pinv recursion must then reproduce the conditional moments of the
    stacked Gaussian to 1e-9 relative -- the bar of tests/test_smoother_reference.py's own brute-force check.  (Measured: states
    8e-15, covariances 5e-14, shocks 5e-15.)"""
    c = K.build("sw17", seg_start=(0, 1, 5), shift=True, a0=True, P0=True, missing=((5, 1), (3, 0), (3, 1), (3, 2), (3, 3)))
    assert np.isnan(c["y"][3]).all() and np.isnan(c["y"][5]).sum() == 1
    conv = dict(jitter_on_P=False, joseph=False)
    for b in range(2):
        segs, fwd, (a, V, e) = _smooth(c, b, conv)
        a2, V2, e2 = brute_force_segmented_smoother(c["y"], segs, c["seg_start"], c["a0"][b], c["P0"][b], c["shift"][b], oracle.JITTER_DEFAULT)
        assert np.isnan(e[0]).all() and np.isnan(e2[0]).all()
        errs = (np.abs(a - a2).max() / np.abs(a2).max(), np.abs(V - V2).max() / np.abs(V2).max(),
                np.abs(e[1:] - e2[1:]).max() / np.abs(e2[1:]).max())
        print("draw", b, "pinv recursion - brute force, relative (states, covs, shocks):", errs)
        assert max(errs) <= 1e-9, errs
        assert np.abs(a - fwd["a_filt"]).max() >= 1e-2 * np.abs(a2).max()  # (smoothing is not trivially the filter)


def _range_against_pinv(c, label, conv=None):
    worst = 0.0
    for b in range(c["T"].shape[0]):
        segs, fwd, (a, V, e) = _smooth(c, b, conv)
        a2, V2, e2, ranks = segmented_range_smoother(fwd, segs, c["seg_start"])
        sa, sp, se = SSC.scales(c, b, fwd)
        errs = (np.abs(a2 - a).max() / sa, np.abs(V2 - V).max() / sp, 0.0 if a.shape[0] < 2 else np.abs(e2[1:] - e[1:]).max() / se)
        print(label, "draw", b, "ranks", ranks, "range form - pinv form / scale (states, covs, shocks):", errs)
        assert np.isnan(e[0]).all() and np.isnan(e2[0]).all()
        assert max(errs) <= 1e-10, (label, b, errs)
        worst = max(worst, *errs)
    return worst, ranks


@pytest.mark.parametrize("name", SSC.ACCURACY_CASES)
def test_range_form_matches_pinv_form(name):
    """The condition on the INPUTS of every case the device is held to: the device's form of the recursion restated in numpy (one
    basis per segment) and the reference's (pinv) agree within 1e-10 x scale -- one decade under the device's bar, so that the
    reference's own noise cannot decide a device test -- and cond_2(F_t) <= 1e4 at every period."""
    print(name, "largest cond_2(F_t):", SSC.check_conditions(name))
    _, ranks = _range_against_pinv(SSC.case(name), name)
    if name in SSC.RANK_CASES:
        assert ranks[1] < ranks[0] and ranks[2] < ranks[0], ranks  # (the shock without variance; the extra zero column)


def test_range_form_matches_pinv_form_under_every_convention():
    """The same condition on the inputs of the device's conventions test: all 48 combinations on the 17-variable case, under the
    missing-data rule of tests/test_gpu_conventions.py."""
    c, full = SSC.case(K.CONVENTION_CASE), SSC.case(K.CONVENTION_CASE_COMPLETE)
    assert c["T"].shape[2] == 17 and len(K.CONVENTIONS) == 48
    worst = max(_range_against_pinv(c if conv["jitter_on_F"] else full, str(conv), conv)[0] for conv in K.CONVENTIONS)
    print("48 conventions, largest figure:", worst)


def test_identical_segments_reproduce_the_plain_smoother():
    """S = 1: ``rts_smoother`` on the oracle's states, exactly.  S = 3 with equal matrices: 1e-12 x scale (the chained filter
    symmetrises the boundary prediction in another order)."""
    one = K.case("s1")
    x = K.draw(one, 0)[0]
    _, ll, stt = oracle.kalman_filter_logp(one["y"], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], return_states=True)
    want = rts_smoother(stt, x["T"], x["R"], x["Q"])
    _, fwd, got = _smooth(one, 0)
    assert np.array_equal(fwd["ll"], ll) and all(np.array_equal(fwd[key], stt[key]) for key in stt)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    segs = [x, x, x]
    fwd3 = segmented_forward(one["y"], segs, (0, 3, 6))
    got3 = segmented_rts_smoother(fwd3, segs, (0, 3, 6))
    sa, sp, se = SSC.scales(one, 0, fwd)
    errs = (np.abs(got3[0] - want[0]).max() / sa, np.abs(got3[1] - want[1]).max() / sp, np.abs(got3[2][1:] - want[2][1:]).max() / se)
    print("S = 3 with equal matrices against rts_smoother / scale:", errs)
    assert max(errs) <= 1e-12


def test_transition_identity_across_boundaries():
    """Without the P jitter the smoothed path is a path of the model: as[t+1] = T_s' (as[t] + [boundary] shift_s') + R_s' eps[t+1]
    with s' = s(t+1), across boundaries as inside segments, to 1e-10 x scale."""
    c = K.build("sw17", seg_start=(0, 1, 5), shift=True, a0=True, P0=True)
    for b in range(2):
        segs, fwd, (a, _, e) = _smooth(c, b, dict(jitter_on_P=False))
        sa = SSC.scales(c, b, fwd)[0]
        worst = 0.0
        for t in range(a.shape[0] - 1):
            s = segment_of(c["seg_start"], t + 1)
            at = a[t] + (c["shift"][b][s] if t + 1 == c["seg_start"][s] else 0.0)
            worst = max(worst, np.abs(a[t + 1] - segs[s]["T"] @ at - segs[s]["R"] @ e[t + 1]).max() / sa)
        print("draw", b, "transition identity / scale:", worst)
        assert worst <= 1e-10


# ---- the front end against a stand-in library ---------------------------------------------------------------------------------------
NB, S, M, KK, P, N = 2, 3, 5, 2, 2, 8
SEG = (0, 3, 6)
ENTRY = "dsge_kalman_smoother_segments_batched"
OUT_ARGS = ("ll_out", "a_pred_out", "a_filt_out", "p_pred_out", "p_filt_out", "a_smooth_out", "p_smooth_out", "eps_smooth_out")


def _model(nb=NB, s=S, m=M, k=KK):
    return np.zeros((nb, s, m, m)), np.zeros((nb, s, m, k))


def _rest(s=S, m=M, k=KK, p=P, n=N):
    return np.ones((s, k)), np.zeros((s, p, m)), np.zeros((n, p))


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _NoCall())


class _Recorder:
    """Stands in for ``_lib.call``: keeps the entries called and the named arguments of the last call."""

    def __init__(self):
        self.entries = []

    def __call__(self, entry, *, host, stream=None, **named):
        self.entries.append(entry)
        self.entry, self.named = entry, named


@pytest.fixture
def recorded(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def test_the_signature_follows_the_likelihood_and_the_abi_version_is_unchanged():
    text = open(os.path.join(ROOT, "include", "dsge_hip.h")).read()
    assert int(dict(re.findall(r"#define\s+(DSGE_[A-Z_0-9]+)\s+(-?\d+)", text))["DSGE_ABI_VERSION"]) == _lib.ABI_VERSION == 19
    sig = [a for a, _ in _lib.SIGNATURES[ENTRY]]
    like = [a for a, _ in _lib.SIGNATURES["dsge_kalman_logp_segments_batched"]]
    cut = like.index("missing_fill") + 1
    assert sig[:cut] == like[:cut]
    assert sig[cut:] == ["rank_tol", "scratch_limit_bytes", "full_cov", *OUT_ARGS, "status_io", "stream"]
    assert [a for a, _ in _lib.SIGNATURES[ENTRY + "_host"]] == sig[:-1]


def test_every_layout_is_read_off_the_shapes(recorded):
    call = batched.kalman_smoother_segments_batched
    T, R = _model()
    q, Z, y = _rest()
    r = call(T, R, q, Z, y, SEG)
    a = recorded.named
    assert recorded.entry == ENTRY
    assert (a["batch"], a["n_seg"], a["m"], a["k"], a["p"], a["T_len"]) == (NB, S, M, KK, P, N)
    assert (a["q_mode"], a["z_batched"], a["d_batched"], a["h_batched"], a["full_cov"]) == (_lib.Q_DIAG_SHARED, 0, 0, 0, False)
    assert (a["rank_tol"], a["scratch_limit_bytes"]) == (0.0, 0)
    assert all(a[key] is None for key in ("d", "Hdiag", "a0", "P0", "shift")) and all(a[key] is not None for key in OUT_ARGS)
    assert isinstance(a["seg_start"], int) and a["seg_start"] != 0  # (a host address, for the device front end too)
    assert sorted(r) == sorted(SSC.KEYS + ("status",))
    assert r["ll"].shape == (NB, N) and r["smoothed_shocks"].shape == (NB, N, KK)
    assert all(r[key].shape == (NB, N, M) for key in ("a_pred", "a_filt", "P_pred", "P_filt", "smoothed_states", "smoothed_covs"))
    assert r["status"].dtype == np.int32 and not r["status"].any()
    r = call(T, R, q, Z, y, SEG, full_covariances=True, rank_tol=1e-9, scratch_limit_bytes=1 << 20)
    a = recorded.named
    assert (a["full_cov"], a["rank_tol"], a["scratch_limit_bytes"]) == (True, 1e-9, 1 << 20)
    assert all(r[key].shape == (NB, N, M, M) for key in ("P_pred", "P_filt", "smoothed_covs"))
    for qq, code in ((np.ones((NB, S, KK)), _lib.Q_DIAG_BATCHED), (np.ones((S, KK, KK)), _lib.Q_FULL_SHARED),
                     (np.ones((NB, S, KK, KK)), _lib.Q_FULL_BATCHED)):
        call(T, R, qq, Z, y, SEG)
        assert recorded.named["q_mode"] == code
    call(T, R, q, np.zeros((NB, S, P, M)), y, SEG, d=np.zeros((NB, S, P)), Hdiag=np.zeros((S, P)), a0=np.zeros((NB, M)),
         P0=np.zeros((NB, M, M)), shift=np.zeros((NB, S, M)), jitter=0.5, missing_fill_value=-1.0)
    a = recorded.named
    assert (a["z_batched"], a["d_batched"], a["h_batched"], a["jitter"], a["missing_fill"]) == (1, 1, 0, 0.5, -1.0)
    assert all(a[key] is not None for key in ("d", "Hdiag", "a0", "P0", "shift"))
    # one output alone: every other pointer is null (without smoothed_covs the covariance recursion is skipped)
    for key, arg in zip(SSC.KEYS, OUT_ARGS):
        r = call(T, R, q, Z, y, SEG, outputs=(key,))
        assert all((recorded.named[x] is not None) == (x == arg) for x in OUT_ARGS), key
        assert all((r[other] is not None) == (other == key) for other in SSC.KEYS), key
    call(*_model(s=1), *_rest(s=1), [0])
    assert recorded.named["n_seg"] == 1
    call(*_model(s=8), *_rest(s=8), np.arange(8, dtype=np.int64))
    assert recorded.named["n_seg"] == 8
    assert batched.segment_smoother_scratch_bytes_per_draw(40, 200, 3) == 8 * (2 * 200 * 1600 + 2 * 200 * 40 + 9 * 48 * 50)


def test_the_fused_front_end_flattens_solves_and_smooths(recorded):
    A = np.zeros((NB, S, M, M))
    D = np.zeros((NB, S, M, KK))
    q, Z, y = _rest()
    for solver, first in (("cycle_reduction", ["dsge_cycle_reduction_batched", "dsge_selection_batched"]),
                          ("gensys", ["dsge_gensys_batched"]), ("backward_direct", ["dsge_backward_direct_batched"])):
        recorded.entries.clear()
        r = batched.solve_kalman_smoother_segments_batched(A, A, A, D, q, Z, y, SEG, solver=solver)
        assert recorded.entries == first + [ENTRY]
        assert r["T"].shape == (NB, S, M, M) and r["R"].shape == (NB, S, M, KK) and r["status"].shape == (NB,)
        assert (recorded.named["batch"], recorded.named["n_seg"], recorded.named["m"], recorded.named["k"]) == (NB, S, M, KK)


def test_every_refusal_comes_before_the_library_is_called(no_library):
    T, R = _model()
    q, Z, y = _rest()
    A, D = np.zeros((NB, S, M, M)), np.zeros((NB, S, M, KK))
    for call, head in ((batched.kalman_smoother_segments_batched, (T, R)), (batched.solve_kalman_smoother_segments_batched, (A, A, A, D))):
        for seg, says in (((), "1 .. 8 segments"), ((1, 3, 6), r"seg_start\[0\] must be 0"), ((0, 3, 3), "strictly increasing"),
                          ((0, 5, 4), "strictly increasing"), ((0, 3, 8), "< T_len = 8"), (None, "required"), ((0, 2.5, 6), "integers")):
            with pytest.raises(ValueError, match=says):
                call(*head, q, Z, y, seg)
        with pytest.raises(ValueError, match="1 .. 8 segments"):
            call(*head, q, Z, np.zeros((12, P)), tuple(range(9)))
        with pytest.raises(ValueError, match="required"):
            call(*head, q, None, y, SEG)
        with pytest.raises(ValueError, match="required"):
            call(*head, q, Z, None, SEG)
        with pytest.raises(ValueError, match="required"):
            call(head[0], None, *head[2:], q, Z, y, SEG)
    call = batched.kalman_smoother_segments_batched
    for kw, says in ((dict(d=np.zeros(P)), "d must be"), (dict(Hdiag=np.zeros((NB, P))), "Hdiag must be"), (dict(a0=np.zeros(M)), "a0 must be"),
                     (dict(P0=np.zeros((NB, M))), "P0 must be"), (dict(shift=np.zeros((NB, M))), "shift must be"),
                     (dict(outputs=("ll", "logp")), "outputs must be among"), (dict(outputs=()), "at least one output"),
                     (dict(scratch_limit_bytes=-1), "scratch_limit_bytes"), (dict(status=np.zeros(3, dtype=np.int32)), "status must be")):
        with pytest.raises(ValueError, match=says):
            call(T, R, q, Z, y, SEG, **kw)
    with pytest.raises(ValueError, match="2 entries, T has 3 segments"):
        call(T, R, q, Z, y, (0, 3))
    with pytest.raises(ValueError, match="cannot infer the layout of Q"):
        call(T, R, np.ones((S + 1, KK)), Z, y, SEG)
    with pytest.raises(ValueError, match="Z must be"):
        call(T, R, q, np.zeros((P, M)), y, SEG)
    with pytest.raises(ValueError, match="T must be"):
        call(T[:, :, :4], R, q, Z, y, SEG)
    with pytest.raises(ValueError, match="at most 64 variables"):
        call(np.zeros((1, 1, 65, 65)), np.zeros((1, 1, 65, 1)), np.ones((1, 1)), np.zeros((1, 2, 65)), y, (0,))
    with pytest.raises(ValueError, match="solver must be"):
        batched.solve_kalman_smoother_segments_batched(A, A, A, D, q, Z, y, SEG, solver="scan_cycle_reduction")


def _c_args(T, R, q, Z, y, seg, n_seg, *, m=M, k=KK, p=P, T_len=N, batch=NB, outputs=True, status=True, q_mode=0):
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    a_s, st = np.zeros((NB, N, M)), np.zeros(NB, dtype=np.int32)
    keep = (a_s, st)
    return keep, [ptr(T), ptr(R), ptr(q), q_mode, ptr(Z), 0, None, 0, None, 0, None, None, None, ptr(y), ptr(seg), n_seg, batch, m, k, p,
                  T_len, 1e-8, -9999.0, 0.0, 0, 0, None, None, None, None, None, ptr(a_s) if outputs else None, None, None,
                  ptr(st) if status else None]


@pytest.mark.parametrize("entry", (ENTRY, ENTRY + "_host"))
def test_the_library_refuses_the_same_before_any_device_is_touched(entry):
    lib = _lib.load()
    fn = getattr(lib, entry)
    tail = [None] if not entry.endswith("_host") else []
    T, R = _model()
    q, Z, y = _rest()
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731

    def rc(*a, **kw):
        keep, args = _c_args(*a, **kw)
        return fn(*args, *tail)

    assert rc(T, R, q, Z, y, i32(0, 3, 6), 0) == _lib.ERR_INVALID and b"n_seg" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(*range(9)), 9) == _lib.ERR_INVALID and b"n_seg" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(1, 3, 6), 3) == _lib.ERR_INVALID and b"seg_start[0]" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(0, 3, 3), 3) == _lib.ERR_INVALID and b"strictly increasing" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(0, 6, 3), 3) == _lib.ERR_INVALID and b"strictly increasing" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(0, 3, 8), 3) == _lib.ERR_INVALID and b"< T_len" in lib.dsge_last_error()
    for missing in range(6):  # T, R, Q, Z, y, seg_start
        a = [T, R, q, Z, y, i32(0, 3, 6)]
        a[missing] = None
        assert rc(*a, 3) == _lib.ERR_INVALID and b"null pointer" in lib.dsge_last_error(), missing
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, outputs=False) == _lib.ERR_INVALID and b"no output" in lib.dsge_last_error()
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, status=False) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, q_mode=4) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, k=M + 1) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, batch=-1) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, m=_lib.MAX_N + 1) == _lib.ERR_TOO_LARGE
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, p=_lib.MAX_P + 1) == _lib.ERR_TOO_LARGE
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, T_len=0) != _lib.ERR_INVALID  # (the list is not held against an empty panel)


def test_no_new_kernel_instantiation_uses_scratch_memory(tmp_path):
    """The storing filter (a translation unit of its own) and the backward pass with the segment switch (next to the plain one):
    the list of breaks is read with constant indices out of the kernel arguments, and neither that nor the stores may turn into a
    private array (scratch) unnoticed."""
    import subprocess

    from geconpy_amd import build

    found = {}
    for src in ("launch_kalman_seg_store.hip", "launch_smooth.hip"):
        out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "a.o"),
                              os.path.join(build.CSRC, src)], cwd=build.CSRC, capture_output=True, text=True, check=True)
        names = re.findall(r"Function Name: (\S+)", out.stderr)
        sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
        assert len(names) == len(sizes)
        found.update(zip(names, sizes))
    store = [n for n in found if "kalman_seg_kernelILb1E" in n]
    back = [n for n in found if "kalman_smoother_kernelILb0ELb1E" in n or "kalman_smoother_kernelILb1ELb1E" in n]
    assert len(store) == 1 and len(back) == 2 and any("ks_seg_status_kernel" in n for n in found)
    assert set(found.values()) == {"0"}, found
