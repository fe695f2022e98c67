"""CPU: the front ends of the gradient across dated structural breaks against a stand-in library (no device): the C signature next
to its neighbours, every refusal before the library is called, the output-selection plumbing, the call sequence of the fused front
end, and the pytensor Op against a stand-in ``pt`` -- including the sum over the batch for inputs the draws share
(docs/design/segmented_gradient.md)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import geconpy_amd.pytensor_ops as ops
from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, S, M, KK, P, N = 2, 3, 5, 2, 2, 8
SEG = (0, 3, 6)
ENTRY = "dsge_kalman_logp_segments_grad_batched"
BAR_ARGS = ("T_bar", "R_bar", "Q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar", "a0_bar", "P0_bar")
KEYS = F.SEGMENT_GRADIENT_OUTPUTS


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
    """Stands in for ``_lib.call``: keeps the entries called and the named arguments of every call."""

    def __init__(self):
        self.entries, self.calls = [], []

    def __call__(self, entry, *, host, stream=None, **named):
        self.entries.append(entry)
        self.calls.append(named)
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
    assert sig[cut:] == ["scratch_limit_bytes", "logp_out", *BAR_ARGS, "status_io", "stream"]
    assert [a for a, _ in _lib.SIGNATURES[ENTRY + "_host"]] == sig[:-1]
    assert re.search(r"int " + ENTRY + r"\(", text) and re.search(r"int " + ENTRY + r"_host\(", text)
    assert ENTRY in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_layout_and_every_selection_of_outputs(recorded):
    call = batched.kalman_logp_segments_grad_batched
    T, R = _model()
    q, Z, y = _rest()
    r = call(T, R, q, Z, y, SEG)
    a = recorded.named
    assert recorded.entry == ENTRY
    assert (a["batch"], a["n_seg"], a["m"], a["k"], a["p"], a["T_len"]) == (NB, S, M, KK, P, N)
    assert (a["q_mode"], a["z_batched"], a["d_batched"], a["h_batched"], a["scratch_limit_bytes"]) == (_lib.Q_DIAG_SHARED, 0, 0, 0, 0)
    assert all(a[key] is None for key in ("d", "Hdiag", "a0", "P0", "shift")) and all(a[key] is not None for key in BAR_ARGS)
    assert isinstance(a["seg_start"], int) and a["seg_start"] != 0  # (a host address, for the device front end too)
    assert sorted(r) == sorted(KEYS + ("logp", "status"))
    shapes = dict(T_bar=(NB, S, M, M), R_bar=(NB, S, M, KK), q_bar=(NB, S, KK), Z_bar=(NB, S, P, M), d_bar=(NB, S, P), h_bar=(NB, S, P),
                  shift_bar=(NB, S, M), a0_bar=(NB, M), P0_bar=(NB, M, M), logp=(NB,), status=(NB,))
    assert {key: r[key].shape for key in r} == shapes  # (per draw, also for the shared q, Z)
    assert r["status"].dtype == np.int32 and not r["status"].any()
    # a full covariance: Q_bar (batch, S, k, k) under its own name, "Q_bar" accepted in outputs and out
    for qq, code in ((np.ones((S, KK, KK)), _lib.Q_FULL_SHARED), (np.ones((NB, S, KK, KK)), _lib.Q_FULL_BATCHED)):
        r = call(T, R, qq, Z, y, SEG, outputs=("Q_bar",))
        assert recorded.named["q_mode"] == code and r["Q_bar"].shape == (NB, S, KK, KK) and "q_bar" not in r
        buf = np.empty((NB, S, KK, KK))
        assert call(T, R, qq, Z, y, SEG, outputs=(), out=dict(Q_bar=buf))["Q_bar"] is buf
    call(T, R, np.ones((NB, S, KK)), Z, y, SEG)
    assert recorded.named["q_mode"] == _lib.Q_DIAG_BATCHED
    call(T, R, q, np.zeros((NB, S, P, M)), y, SEG, d=np.zeros((NB, S, P)), Hdiag=np.zeros((S, P)), a0=np.zeros((NB, M)),
         P0=np.zeros((NB, M, M)), shift=np.zeros((NB, S, M)), jitter=0.5, missing_fill_value=-1.0, scratch_limit_bytes=1 << 20)
    a = recorded.named
    assert (a["z_batched"], a["d_batched"], a["h_batched"], a["jitter"], a["missing_fill"], a["scratch_limit_bytes"]) == (1, 1, 0, 0.5, -1.0, 1 << 20)
    assert all(a[key] is not None for key in ("d", "Hdiag", "a0", "P0", "shift"))
    # one output alone: every other cotangent pointer is null, logp always goes
    for key, arg in zip(KEYS, BAR_ARGS):
        r = call(T, R, q, Z, y, SEG, outputs=(key,))
        assert all((recorded.named[x] is not None) == (x == arg) for x in BAR_ARGS), key
        assert all((r[other] is not None) == (other == key) for other in KEYS) and recorded.named["logp_out"] is not None
    r = call(T, R, q, Z, y, SEG, outputs=())
    assert all(recorded.named[x] is None for x in BAR_ARGS) and r["logp"].shape == (NB,)
    # out=: the buffers are used and returned
    out = dict(logp=np.empty(NB), T_bar=np.empty((NB, S, M, M)))
    r = call(T, R, q, Z, y, SEG, outputs=("d_bar",), out=out)
    assert r["logp"] is out["logp"] and r["T_bar"] is out["T_bar"] and r["d_bar"] is not None and r["R_bar"] is None
    assert batched.segment_gradient_scratch_bytes_per_draw(40, 200, 3) == 8 * (2 * 200 * 1600 + 2 * 200 * 40 + 2 * 3 * 1600)


def test_the_fused_front_end_solves_differentiates_and_pulls_back(recorded):
    A, D = np.zeros((NB, S, M, M)), np.zeros((NB, S, M, KK))
    q, Z, y = _rest()
    for solver, first in (("cycle_reduction", ["dsge_cycle_reduction_batched", "dsge_selection_batched"]), ("gensys", ["dsge_gensys_batched"])):
        recorded.entries.clear()
        recorded.calls.clear()
        with np.errstate(all="ignore"):  # (the stand-in fills nothing: the arithmetic between the calls runs on empty buffers)
            r = batched.solve_kalman_logp_segments_grad_batched(A, A, A, D, q, Z, y, SEG, solver=solver, outputs=("d_bar",))
        assert recorded.entries == first + [ENTRY, "dsge_selection_adjoints_batched", "dsge_policy_adjoints_batched"]
        grad, sel, pol = recorded.calls[-3:]
        assert grad["T_bar"] is not None and grad["R_bar"] is not None and grad["d_bar"] is not None and grad["Z_bar"] is None
        assert (grad["batch"], grad["n_seg"], grad["m"], grad["k"]) == (NB, S, M, KK)
        assert (sel["batch"], sel["n"], sel["k"]) == (NB * S, M, KK) and (pol["batch"], pol["n"]) == (NB * S, M)
        assert pol["T_bar"] not in (grad["T_bar"], sel["T_bar"])  # (the sum of the two, a buffer of its own)
        for key, shape in (("A_bar", (NB, S, M, M)), ("B_bar", (NB, S, M, M)), ("C_bar", (NB, S, M, M)), ("D_bar", (NB, S, M, KK)),
                           ("T", (NB, S, M, M)), ("R", (NB, S, M, KK)), ("T_bar", (NB, S, M, M)), ("d_bar", (NB, S, P)), ("status", (NB,))):
            assert r[key].shape == shape, key
        assert r["Z_bar"] is None


def test_a_failed_draw_of_the_fused_front_end_is_ored_and_zeroed(monkeypatch):
    """The stand-in fills the outputs: the solver fails segment 1 of draw 1, the policy adjoint segment 2 of draw 0's neighbour
    draw 1 again with another bit -- draw 1 gets the OR, -inf and zeros, draw 0 keeps what the entries wrote."""
    def fake(entry, *, host, stream=None, **named):
        def view(key, shape, dtype=np.float64):
            ctype = ctypes.c_double if dtype == np.float64 else ctypes.c_int32
            return np.ctypeslib.as_array(ctypes.cast(named[key], ctypes.POINTER(ctype)), shape=shape)

        if entry == "dsge_cycle_reduction_batched":
            st = view("status", (NB * S,), np.int32)
            st[:] = 0
            st[1 * S + 1] = _lib.ST_NOT_CONVERGED
            view("T_out", (NB * S, M, M))[:] = 0.0
        elif entry == "dsge_selection_batched":
            view("R_out", (NB * S, M, KK))[:] = 0.0
        elif entry == ENTRY:
            st = view("status_io", (NB,), np.int32)
            view("logp_out", (NB,))[:] = np.where(st != 0, -np.inf, -3.0)
            for key, shape in (("T_bar", (NB, S, M, M)), ("R_bar", (NB, S, M, KK)), ("d_bar", (NB, S, P))):
                view(key, shape)[:] = np.where(st != 0, 0.0, 2.0).reshape((NB,) + (1,) * (len(shape) - 1))
        elif entry == "dsge_selection_adjoints_batched":
            for key, shape in (("B_bar", (NB * S, M, M)), ("C_bar", (NB * S, M, M)), ("T_bar", (NB * S, M, M)), ("D_bar", (NB * S, M, KK))):
                view(key, shape)[:] = 1.0
        elif entry == "dsge_policy_adjoints_batched":
            assert np.array_equal(view("T_bar", (NB * S, M, M))[:S], np.full((S, M, M), 3.0))  # (2 from the filter + 1 from R)
            for key in ("A_bar", "B_bar", "C_bar"):
                view(key, (NB * S, M, M))[:] = np.nan
                view(key, (NB * S, M, M))[:S] = 5.0
            st = view("status", (NB * S,), np.int32)
            st[:] = 0
            st[1 * S + 2] = _lib.ST_NAN
    monkeypatch.setattr(_lib, "call", fake)
    A, D = np.zeros((NB, S, M, M)), np.zeros((NB, S, M, KK))
    q, Z, y = _rest()
    r = batched.solve_kalman_logp_segments_grad_batched(A, A, A, D, q, Z, y, SEG, outputs=("d_bar",))
    assert list(r["status"]) == [0, _lib.ST_NOT_CONVERGED] and list(r["logp"]) == [-3.0, -np.inf]
    for key in ("A_bar", "B_bar", "C_bar", "D_bar", "T_bar", "R_bar", "d_bar"):
        assert not r[key][1].any() and np.isfinite(r[key]).all(), key
    assert (r["A_bar"][0] == 5.0).all() and (r["B_bar"][0] == 6.0).all() and (r["C_bar"][0] == 6.0).all() and (r["D_bar"][0] == 1.0).all()


def test_every_refusal_comes_before_the_library_is_called(no_library):
    T, R = _model()
    q, Z, y = _rest()
    A, D = np.zeros((NB, S, M, M)), np.zeros((NB, S, M, KK))
    for call, head in ((batched.kalman_logp_segments_grad_batched, (T, R)), (batched.solve_kalman_logp_segments_grad_batched, (A, A, A, D))):
        for seg, says in (((), "1 .. 8 segments"), ((1, 3, 6), r"seg_start\[0\] must be 0"), ((0, 3, 3), "strictly increasing"),
                          ((0, 5, 4), "strictly increasing"), ((0, 3, 8), "< T_len = 8"), (None, "required"), ((0, 2.5, 6), "integers")):
            with pytest.raises(ValueError, match=says):
                call(*head, q, Z, y, seg)
        with pytest.raises(ValueError, match="1 .. 8 segments"):
            call(*head, q, Z, np.zeros((12, P)), tuple(range(9)))
        with pytest.raises(ValueError, match="required"):
            call(*head, q, None, y, SEG)
    call = batched.kalman_logp_segments_grad_batched
    for kw, says in ((dict(d=np.zeros(P)), "d must be"), (dict(Hdiag=np.zeros((NB, P))), "Hdiag must be"), (dict(a0=np.zeros(M)), "a0 must be"),
                     (dict(P0=np.zeros((NB, M))), "P0 must be"), (dict(shift=np.zeros((NB, M))), "shift must be"),
                     (dict(outputs=("T_bar", "logp")), "outputs must be among"), (dict(scratch_limit_bytes=-1), "scratch_limit_bytes"),
                     (dict(status=np.zeros(3, dtype=np.int32)), "status must be"), (dict(q_mode="full"), "q_mode needs"),
                     (dict(out=dict(T_bar=np.zeros((NB, M, M)))), "an output buffer")):
        with pytest.raises(ValueError, match=says):
            call(T, R, q, Z, y, SEG, **kw)
    with pytest.raises(ValueError, match="2 entries, T has 3 segments"):
        call(T, R, q, Z, y, (0, 3))
    with pytest.raises(ValueError, match="T must be"):
        call(T[:, :, :, :4], R, q, Z, y, SEG)
    with pytest.raises(ValueError, match="at most 64 variables"):
        call(np.zeros((1, 1, 65, 65)), np.zeros((1, 1, 65, 1)), np.ones((1, 1)), np.zeros((1, P, 65)), y, (0,))
    fused = batched.solve_kalman_logp_segments_grad_batched
    with pytest.raises(ValueError, match="backward_direct has no adjoint"):
        fused(A, A, A, D, q, Z, y, SEG, solver="backward_direct")
    with pytest.raises(ValueError, match="at most 56 variables"):
        fused(np.zeros((1, 1, 57, 57)), np.zeros((1, 1, 57, 57)), np.zeros((1, 1, 57, 57)), np.zeros((1, 1, 57, 1)), np.ones((1, 1)),
              np.zeros((1, P, 57)), y, (0,))
    with pytest.raises(ValueError, match="solver must be"):
        fused(A, A, A, D, q, Z, y, SEG, solver="newton")


# ---- the Op against a stand-in pytensor ----------------------------------------------------------------------------------------------
class _Type:
    def __init__(self, dtype, shape):
        self.dtype, self.shape, self.ndim = dtype, tuple(shape), len(shape)


class _Var:
    """A symbolic value that knows its shape and how it was made: enough for make_node and pullback."""

    def __init__(self, name, dtype, shape, owner=None, made=None):
        self.name, self.type, self.owner, self.made = name, _Type(dtype, shape), owner, made

    def reshape(self, shape):
        known = [s for s in shape if s != -1]
        size = int(np.prod(self.type.shape)) // max(int(np.prod(known)), 1)
        return _Var("reshape", self.type.dtype, tuple(size if s == -1 else s for s in shape), made=("reshape", self))

    def __mul__(self, other):
        return _Var("mul", "float64", np.broadcast_shapes(self.type.shape, other.type.shape), made=("mul", self, other))

    def sum(self, axis):
        shape = tuple(s for i, s in enumerate(self.type.shape) if i != axis)
        return _Var("sum", self.type.dtype, shape, made=("sum", self, axis))


class _Apply:
    def __init__(self, op, inputs, outputs):
        self.op, self.inputs, self.outputs = op, list(inputs), list(outputs)
        for o in outputs:
            o.owner = self


@pytest.fixture()
def surface(monkeypatch):
    if ops.available():
        pytest.skip("pytensor is installed: the real classes are exercised by pytensor itself")
    fake = types.SimpleNamespace(as_tensor=lambda x: x if isinstance(x, _Var) else _Var("const", "float64", np.shape(x)),
                                 tensor=lambda name, dtype="float64", shape=(): _Var(name, dtype, shape))
    monkeypatch.setattr(ops, "pt", fake)
    monkeypatch.setattr(ops, "Apply", _Apply)
    monkeypatch.setattr(ops, "_HAVE_PYTENSOR", True)
    monkeypatch.setattr(ops.Op, "__init__", lambda self: None, raising=False)
    return ops


def _inputs(shared):
    lead = () if shared else (NB,)
    return [_Var("T", "float64", (NB, S, M, M)), _Var("R", "float64", (NB, S, M, KK)), _Var("q", "float64", lead + (S, KK)),
            _Var("Z", "float64", lead + (S, P, M)), _Var("d", "float64", lead + (S, P)), _Var("Hdiag", "float64", lead + (S, P)),
            _Var("shift", "float64", (NB, S, M))]


def test_the_op_and_its_pullback(surface):
    y = np.arange(N * P, dtype=np.float64).reshape(N, P)
    op = surface.HipKalmanLogpSegments(y, SEG, q_mode="diag", conventions=dict(ll_constant="one"))
    assert op.__props__ == ("y_shape", "y_bytes", "seg_start", "q_mode", "jitter", "missing_fill_value", "conventions")
    assert op.seg_start == SEG and np.array_equal(op.y, y) and hash(op.y_bytes) == hash(y.tobytes())
    with pytest.raises(ValueError, match="strictly increasing"):
        surface.HipKalmanLogpSegments(y, (0, 3, 3))
    with pytest.raises(ValueError, match="q_mode must be"):
        surface.HipKalmanLogpSegments(y, SEG, q_mode="dense")
    for shared in (True, False):
        inputs = _inputs(shared)
        op = surface.HipKalmanLogpSegments(y, SEG, q_mode="diag" if shared else "diag_batched")
        node = op.make_node(*inputs)
        logp = node.outputs[0]
        assert logp.type.shape == (NB,) and op.infer_shape(None, node, [v.type.shape for v in inputs]) == [(NB,)]
        g = _Var("g", "float64", (NB,))
        grads = op.pullback(inputs, [logp], [g])
        assert [x.type.shape for x in grads] == [v.type.shape for v in inputs]
        for v, x in zip(inputs, grads):
            lacks_draw_axis = shared and v.name in ("q", "Z", "d", "Hdiag")
            assert (x.made[0] == "sum" and x.made[2] == 0) == lacks_draw_axis, v.name  # (shared: the sum over the batch)
            prod = x.made[1] if lacks_draw_axis else x
            bar, w = prod.made[1], prod.made[2]
            assert isinstance(bar.owner.op, surface.HipKalmanLogpSegmentsGrad) and bar.type.shape == ((NB,) + v.type.shape if lacks_draw_axis else v.type.shape)
            assert w.made == ("reshape", g) and w.type.shape == (NB,) + (1,) * (bar.type.ndim - 1)
            gop = bar.owner.op
            assert (gop.seg_start, gop.q_mode, gop.y_bytes) == (op.seg_start, op.q_mode, op.y_bytes) and bar.owner.inputs == inputs
        gnode = grads[0].made[1].owner
        assert [o.name for o in gnode.outputs] == ["T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar"]
        assert [o.type.shape for o in gnode.outputs] == [(NB, S, M, M), (NB, S, M, KK), (NB, S, KK), (NB, S, P, M), (NB, S, P), (NB, S, P),
                                                         (NB, S, M)]
        assert gnode.op.infer_shape(None, gnode, [v.type.shape for v in inputs]) == [o.type.shape for o in gnode.outputs]
    # a full covariance: Q_bar (batch, S, k, k); three axes without q_mode are ambiguous
    full = _inputs(True)
    full[2] = _Var("q", "float64", (S, KK, KK))
    gnode = surface.HipKalmanLogpSegmentsGrad(y, SEG, q_mode="full").make_node(*full)
    assert gnode.outputs[2].type.shape == (NB, S, KK, KK)
    with pytest.raises(ValueError, match="pass q_mode"):
        surface.HipKalmanLogpSegmentsGrad(y, SEG).make_node(*full)


def test_perform_calls_the_front_ends(monkeypatch):
    y = np.zeros((N, P))
    seen = {}

    def logp(T, R, q, Z, y_, seg, **kw):
        seen["logp"] = (seg, kw)
        return dict(logp=np.full(NB, -1.0))

    def grad(T, R, q, Z, y_, seg, **kw):
        seen["grad"] = (seg, kw)
        return {key: np.full(3, i) for i, key in enumerate(("T_bar", "R_bar", "Q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar"))}

    monkeypatch.setattr(batched, "kalman_logp_segments_batched", logp)
    monkeypatch.setattr(batched, "kalman_logp_segments_grad_batched", grad)
    arrays = [np.zeros(1)] * 7
    cell = [[None]]
    ops.HipKalmanLogpSegments(y, SEG, q_mode="full", jitter=1e-7).perform(None, arrays, cell)
    assert (cell[0][0] == -1.0).all() and seen["logp"][0] == SEG
    assert seen["logp"][1]["q_mode"] == "full" and seen["logp"][1]["jitter"] == 1e-7 and seen["logp"][1]["outputs"] == ("logp",)
    cells = [[None] for _ in range(7)]
    ops.HipKalmanLogpSegmentsGrad(y, SEG, q_mode="full").perform(None, arrays, cells)
    assert [int(c[0][0]) for c in cells] == list(range(7))  # (Q_bar of a full covariance lands in the q_bar slot)
    assert "P0_bar" not in seen["grad"][1]["outputs"] and seen["grad"][1]["q_mode"] == "full"
