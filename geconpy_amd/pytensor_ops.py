"""pytensor Ops backed by libdsge_hip.so -- the drop-in surface for gEconpy's solver Ops.

Mirrors, for the cycle-reduction path, the interface of
``gEconpy/solvers/cycle_reduction.py``: ``CycleReductionWrapper`` (``__props__ = ("max_iter",
"tol")``, ``gufunc_signature = "(n,n),(n,n),(n,n)->(n,n)"``, ``make_node`` / ``infer_shape`` /
``perform`` / ``pullback`` contract, :186-213) and ``cycle_reduction_pt`` (:216-219), plus
``pt_compute_selection_matrix`` (``gEconpy/solvers/shared.py:74-75``).  On top of that it adds
what the reference does not have: explicitly batched Ops (leading draw axis, ONE kernel launch
per batch) and the fused ``A,B,C,D -> logp`` Op, and it registers a vectorisation rule so that
``pytensor.graph.replace.vectorize_graph`` / ``Blockwise`` turn the per-draw Op into the batched
one instead of a Python loop over draws (the hook of ``statespace.py:1217-1303``).

pytensor is imported lazily: this module can be imported without it (``available()`` tells),
and the engine is fully usable through ``geconpy_amd.batched`` / ``geconpy_amd.engine`` alone.
Registration happens by import side effect, the same pattern as ``gEconpy/__init__.py:33-35``.
"""
from __future__ import annotations

import numpy as np

from . import _lib, batched

try:  # pragma: no cover - exercised only where pytensor is installed
    import pytensor.tensor as pt
    from pytensor.graph.basic import Apply
    from pytensor.graph.op import Op

    _HAVE_PYTENSOR = True
except Exception:  # noqa: BLE001  (ImportError or a broken install)
    pt = None
    Apply = None
    _HAVE_PYTENSOR = False

    class Op:  # minimal base so that the classes exist (perform() is callable) without pytensor
        def __call__(self, *inputs):
            node = self.make_node(*inputs)  # raises ImportError through _require() unless a tensor module is bound
            return node.outputs[0] if len(node.outputs) == 1 else list(node.outputs)


def available() -> bool:
    return _HAVE_PYTENSOR


def _require():
    if not _HAVE_PYTENSOR:
        raise ImportError("pytensor is not installed; use geconpy_amd.batched / geconpy_amd.engine directly")


def _floatx():
    """``pytensor.config.floatX``: the dtype ``pt.tensor("T", shape=...)`` gets in ``GensysWrapper.make_node`` (gensys.py:646),
    which declares no dtype; float64 where pytensor is not importable."""
    try:
        import pytensor  # noqa: PLC0415

        return str(pytensor.config.floatX)
    except Exception:  # noqa: BLE001
        return "float64"


def _as3(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x[None] if x.ndim == 2 else x


def _out_dtype(*dtypes):
    """Output dtype of a solver Op: pytensor's ``linalg_output_dtype`` (what ``CycleReductionWrapper.make_node`` uses,
    cycle_reduction.py:197) when this pytensor has it; otherwise its rule restated -- float32 only if every input is
    float32 (or narrower), float64 else.  The kernels always compute in float64; ``perform`` casts the result
    (``np.asarray(T, dtype=node.outputs[0].type.dtype)``, cycle_reduction.py:210)."""
    try:
        from pytensor.tensor.linalg.dtype_utils import linalg_output_dtype  # noqa: PLC0415

        return linalg_output_dtype(*dtypes)
    except Exception:  # noqa: BLE001
        return "float32" if dtypes and all(np.dtype(d).itemsize <= 4 and np.dtype(d).kind == "f" for d in dtypes) else "float64"


class HipCycleReduction(Op):
    """Drop-in for ``CycleReductionWrapper``: ``T = Op(A, B, C)`` with (n, n) inputs.

    ``perform`` calls ``dsge_cycle_reduction_batched_host`` with batch = 1.  Like the reference's
    numpy ``perform`` it has no convergence output; unlike it (which stores ``None``) a failed solve
    yields the zero matrix, i.e. the njit semantics of cycle_reduction.py:181.
    """

    __props__ = ("max_iter", "tol")
    gufunc_signature = "(n,n),(n,n),(n,n)->(n,n)"

    def __init__(self, max_iter=1000, tol=1e-9):
        self.max_iter = int(max_iter)
        self.tol = tol
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C)]
        o_dtype = _out_dtype(*(inp.type.dtype for inp in inputs))
        outputs = [pt.tensor("T", dtype=o_dtype, shape=inputs[0].type.shape)]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        n = input_shapes[0][0]
        return [(n, n)]

    def perform(self, node, inputs, outputs):
        A, B, C = (_as3(x) for x in inputs)
        T, _status, _n_iter = batched.cycle_reduction_batched(A, B, C, max_iter=self.max_iter, tol=self.tol)
        o_dtype = node.outputs[0].type.dtype if node is not None else "float64"
        outputs[0][0] = np.asarray(T[0], dtype=o_dtype)

    def pullback(self, inputs, outputs, cotangents):
        # Same contract as _linear_policy_jvp (cycle_reduction.py:117-124): cotangents of (A, B, C)
        # from the cotangent of T, computed on the device (doubling solve of the adjoint Stein
        # equation) instead of the reference's n^2 x n^2 Kronecker solve (shared.py:53-71).
        _A, B, C = inputs
        return list(HipPolicyAdjoint()(B, C, outputs[0], cotangents[0]))


class HipPolicyAdjoint(Op):
    """``A_bar, B_bar, C_bar = Op(B, C, T, T_bar)`` -- ``o1_policy_function_adjoints``
    (gEconpy/solvers/shared.py:12-71) for (n, n) or (batch, n, n) inputs."""

    __props__ = ()
    gufunc_signature = "(n,n),(n,n),(n,n),(n,n)->(n,n),(n,n),(n,n)"

    def make_node(self, B, C, T, T_bar):
        _require()
        inputs = [pt.as_tensor(x) for x in (B, C, T, T_bar)]
        outputs = [pt.tensor(name, dtype="float64", shape=inputs[0].type.shape) for name in ("A_bar", "B_bar", "C_bar")]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        return [input_shapes[0]] * 3

    def perform(self, node, inputs, outputs):
        squeeze = np.ndim(inputs[0]) == 2
        B, C, T, T_bar = (_as3(x) for x in inputs)
        Ab, Bb, Cb, _status = batched.policy_adjoints_batched(B, C, T, T_bar)
        for cell, val in zip(outputs, (Ab, Bb, Cb)):
            cell[0] = val[0] if squeeze else val


class HipCycleReductionBatched(Op):
    """``T, status = Op(A, B, C)`` with (batch, n, n) inputs: one launch for all draws."""

    __props__ = ("max_iter", "tol")

    def __init__(self, max_iter=1000, tol=1e-9):
        self.max_iter = int(max_iter)
        self.tol = tol
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C)]
        outputs = [
            pt.tensor("T", dtype="float64", shape=inputs[0].type.shape),
            pt.tensor("status", dtype="int32", shape=inputs[0].type.shape[:1]),
        ]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        b, n, _ = input_shapes[0]
        return [(b, n, n), (b,)]

    def perform(self, node, inputs, outputs):
        T, status, _n_iter = batched.cycle_reduction_batched(*inputs, max_iter=self.max_iter, tol=self.tol)
        outputs[0][0] = T
        outputs[1][0] = status


class HipSelection(Op):
    """``R = -(C T + B)^-1 D`` for (n, n)/(n, k) or batched inputs (shared.py:74-75)."""

    __props__ = ()
    gufunc_signature = "(n,n),(n,n),(n,k),(n,n)->(n,k)"

    def make_node(self, B, C, D, T):
        _require()
        inputs = [pt.as_tensor(x) for x in (B, C, D, T)]
        outputs = [pt.tensor("R", dtype="float64", shape=inputs[2].type.shape)]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        return [input_shapes[2]]

    def perform(self, node, inputs, outputs):
        squeeze = np.ndim(inputs[0]) == 2
        B, C, D, T = (_as3(x) for x in inputs)
        R = batched.selection_batched(B, C, D, T)
        outputs[0][0] = R[0] if squeeze else R

    def pullback(self, inputs, outputs, cotangents):
        # The reference's R is plain differentiable pytensor (-pt.linalg.solve(C @ T + B, D), shared.py:74-75), so
        # pytensor.grad flows through it into B, C, D and T; same rule here, as one launch:
        # G = -(C T + B)^-T R_bar, B_bar = G R', C_bar = G R' T', D_bar = G, T_bar = C' G R'.
        B, C, _D, T = inputs
        B_bar, C_bar, D_bar, T_bar = HipSelectionAdjoint()(B, C, T, outputs[0], cotangents[0])
        return [B_bar, C_bar, D_bar, T_bar]


class HipSelectionAdjoint(Op):
    """``B_bar, C_bar, D_bar, T_bar = Op(B, C, T, R, R_bar)``: reverse mode of ``R = -(C T + B)^-1 D``
    (``dsge_selection_adjoints_batched``), for (n, n)/(n, k) or batched inputs."""

    __props__ = ()
    gufunc_signature = "(n,n),(n,n),(n,n),(n,k),(n,k)->(n,n),(n,n),(n,k),(n,n)"

    def make_node(self, B, C, T, R, R_bar):
        _require()
        inputs = [pt.as_tensor(x) for x in (B, C, T, R, R_bar)]
        sq, sk = inputs[0].type.shape, inputs[3].type.shape
        outputs = [pt.tensor("B_bar", dtype="float64", shape=sq), pt.tensor("C_bar", dtype="float64", shape=sq),
                   pt.tensor("D_bar", dtype="float64", shape=sk), pt.tensor("T_bar", dtype="float64", shape=sq)]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        return [input_shapes[0], input_shapes[0], input_shapes[3], input_shapes[0]]

    def perform(self, node, inputs, outputs):
        squeeze = np.ndim(inputs[0]) == 2
        B, C, T, R, R_bar = (_as3(x) for x in inputs)
        res = batched.selection_adjoints_batched(B, C, T, R, R_bar)
        for cell, val in zip(outputs, res):
            cell[0] = val[0] if squeeze else val


def _conventions_prop(conventions):
    """Hashable form of the ``conventions`` prop of the logp Ops: None, or the sorted items of the keyword arguments of
    ``_lib.filter_conventions`` (validated here, so that a misspelt switch fails when the Op is built)."""
    if conventions is None:
        return None
    items = dict(conventions)
    _lib.filter_conventions(**items)
    return tuple(sorted(items.items()))


def _conventions_options(prop):
    return None if prop is None else _lib.filter_conventions(**dict(prop))


class HipSolveKalmanLogp(Op):
    """Fused per-draw log-likelihood: ``logp, status = Op(A, B, C, D, q, Z, y, d, Hdiag)``.

    A,B,C: (batch, n, n); D: (batch, n, k); q: (batch, k) shock variances (the diagonal of
    ``state_cov``, statespace.py:240-258); Z: (p, n); y: (T_len, p); d, Hdiag: (p,).  Evaluates
    what ``_setup_policy_matrices`` + ``make_symbolic_graph`` + the Kalman scan compute
    (statespace.py:197-222, 725-820, 1151-1157) for all draws in one call; failed draws give -inf.
    """

    __props__ = ("solver", "tol", "max_iter", "jitter", "missing_fill_value", "filter_type", "conventions")

    def __init__(self, solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=batched.JITTER_DEFAULT,
                 missing_fill_value=batched.MISSING_FILL, filter_type="standard", conventions=None):
        batched.check_filter_type(filter_type)  # (build.py:577: only the default filter is built; the others raise here)
        # third-party conventions of the filter step (pymc_extras; dsge_options, ABI 8): None = the library defaults, or the
        # keyword arguments of _lib.filter_conventions (a dict; kept as a sorted tuple: Op props must hash)
        self.conventions = _conventions_prop(conventions)
        self.solver = solver
        self.tol = tol
        self.max_iter = int(max_iter)
        self.jitter = jitter
        self.missing_fill_value = missing_fill_value
        self.filter_type = filter_type
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C, D, q, Z, y, d, Hdiag):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C, D, q, Z, y, d, Hdiag)]
        b = inputs[0].type.shape[:1]
        outputs = [pt.tensor("logp", dtype="float64", shape=b), pt.tensor("status", dtype="int32", shape=b)]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        b = input_shapes[0][0]
        return [(b,), (b,)]

    def perform(self, node, inputs, outputs):
        A, B, C, D, q, Z, y, d, Hdiag = inputs
        out = batched.solve_kalman_logp_batched(
            A, B, C, D, q, Z, y, d=d, Hdiag=Hdiag, q_mode="diag_batched", solver=self.solver, tol=self.tol,
            max_iter=self.max_iter, jitter=self.jitter, missing_fill_value=self.missing_fill_value,
            options=_conventions_options(self.conventions),
        )
        outputs[0][0] = out["logp"]
        outputs[1][0] = out["status"]

    def pullback(self, inputs, outputs, cotangents):
        """Reverse mode through the whole fused evaluation on the device (dsge_solve_kalman_logp_grad_batched):
        cotangents of A, B, C, D, q, d, Hdiag; Z and y are treated as constants of the model (no cotangent --
        gEconpy's selector design matrix and the data)."""
        from pytensor.gradient import disconnected_type  # noqa: PLC0415

        A, B, C, D, q, Z, y, d, Hdiag = inputs
        g_logp = cotangents[0]
        grads = HipSolveKalmanLogpGrad(solver=self.solver, tol=self.tol, max_iter=self.max_iter, jitter=self.jitter,
                                       missing_fill_value=self.missing_fill_value,
                                       conventions=self.conventions)(A, B, C, D, q, Z, y, d, Hdiag)
        A_bar, B_bar, C_bar, D_bar, q_bar, d_bar, h_bar = grads
        w3, w2 = g_logp[:, None, None], g_logp[:, None]
        # d / Hdiag are shared across draws: (p,) inputs receive the sum over the batch
        d_g = (w2 * d_bar).sum(axis=0) if d.type.ndim == 1 else w2 * d_bar
        h_g = (w2 * h_bar).sum(axis=0) if Hdiag.type.ndim == 1 else w2 * h_bar
        return [w3 * A_bar, w3 * B_bar, w3 * C_bar, w3 * D_bar, w2 * q_bar, disconnected_type(), disconnected_type(), d_g, h_g]


class HipSolveKalmanLogpGrad(Op):
    """Cotangents of the fused logp Op: ``A_bar, B_bar, C_bar, D_bar, q_bar, d_bar, h_bar = Op(A, B, C, D, q, Z, y, d,
    Hdiag)`` per draw (for a unit cotangent of logp), computed by the device's reverse sweep."""

    __props__ = ("solver", "tol", "max_iter", "jitter", "missing_fill_value", "conventions")

    def __init__(self, solver="cycle_reduction", tol=1e-6, max_iter=50, jitter=batched.JITTER_DEFAULT,
                 missing_fill_value=batched.MISSING_FILL, conventions=None):
        self.conventions = _conventions_prop(conventions)
        self.solver = solver
        self.tol = tol
        self.max_iter = int(max_iter)
        self.jitter = jitter
        self.missing_fill_value = missing_fill_value
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C, D, q, Z, y, d, Hdiag):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C, D, q, Z, y, d, Hdiag)]
        A_, D_, q_ = inputs[0], inputs[3], inputs[4]
        b = A_.type.shape[:1]
        p = inputs[6].type.shape[-1:]
        outputs = [pt.tensor("A_bar", dtype="float64", shape=A_.type.shape), pt.tensor("B_bar", dtype="float64", shape=A_.type.shape),
                   pt.tensor("C_bar", dtype="float64", shape=A_.type.shape), pt.tensor("D_bar", dtype="float64", shape=D_.type.shape),
                   pt.tensor("q_bar", dtype="float64", shape=q_.type.shape), pt.tensor("d_bar", dtype="float64", shape=b + p),
                   pt.tensor("h_bar", dtype="float64", shape=b + p)]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        sA, _sB, _sC, sD, sq, _sZ, sy, _sd, _sh = input_shapes
        return [sA, sA, sA, sD, sq, (sA[0], sy[1]), (sA[0], sy[1])]

    def perform(self, node, inputs, outputs):
        A, B, C, D, q, Z, y, d, Hdiag = inputs
        out = batched.solve_kalman_logp_grad_batched(A, B, C, D, q, Z, y, d=d, Hdiag=Hdiag, solver=self.solver,
                                                     tol=self.tol, max_iter=self.max_iter, jitter=self.jitter,
                                                     missing_fill_value=self.missing_fill_value,
                                                     options=_conventions_options(self.conventions))
        for cell, key in zip(outputs, ("A_bar", "B_bar", "C_bar", "D_bar", "q_bar", "d_bar", "h_bar")):
            cell[0] = out[key]


class _SegmentsOp(Op):
    """What the two Ops across dated breaks share: the data, the break dates, the conventions and the layout of the shock
    covariance are PROPS (constants of the model; ``y`` is kept as bytes so that the Op hashes), the system matrices are inputs."""

    __props__ = ("y_shape", "y_bytes", "seg_start", "q_mode", "jitter", "missing_fill_value", "conventions")

    def __init__(self, y, seg_start, q_mode=None, jitter=batched.JITTER_DEFAULT, missing_fill_value=batched.MISSING_FILL,
                 conventions=None):
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2:
            raise ValueError(f"y must be (T_len, p); got {y.shape}")
        self.y_shape, self.y_bytes = tuple(y.shape), y.tobytes()
        self.seg_start = tuple(int(s) for s in batched.F.segment_starts(seg_start, y.shape[0]))
        if q_mode is not None and q_mode not in batched.F.Q_MODES:
            raise ValueError(f"q_mode must be one of {tuple(batched.F.Q_MODES)} or None; got {q_mode!r}")
        self.q_mode = q_mode
        self.jitter = jitter
        self.missing_fill_value = missing_fill_value
        self.conventions = _conventions_prop(conventions)
        if _HAVE_PYTENSOR:
            super().__init__()

    @property
    def y(self):
        return np.frombuffer(self.y_bytes, dtype=np.float64).reshape(self.y_shape)

    def _kwargs(self):
        return dict(q_mode=self.q_mode, jitter=self.jitter, missing_fill_value=self.missing_fill_value,
                    options=_conventions_options(self.conventions))


class HipKalmanLogpSegments(_SegmentsOp):
    """Log-likelihood across dated structural breaks per draw: ``logp = Op(T, R, q, Z, d, Hdiag, shift)``
    (``batched.kalman_logp_segments_batched``; a0 = 0 and the stationary P0 of segment 0).  T: (batch, S, m, m); R: (batch, S, m, k);
    q: (S, k), (batch, S, k), (S, k, k) or (batch, S, k, k); Z: (S, p, m) or (batch, S, p, m); d, Hdiag: (S, p) or (batch, S, p);
    shift: (batch, S, m).  Failed draws give -inf.  ``pullback`` runs the device's reverse sweep (``HipKalmanLogpSegmentsGrad``)."""

    def make_node(self, T, R, q, Z, d, Hdiag, shift):
        _require()
        inputs = [pt.as_tensor(x) for x in (T, R, q, Z, d, Hdiag, shift)]
        return Apply(self, inputs, [pt.tensor("logp", dtype="float64", shape=inputs[0].type.shape[:1])])

    def infer_shape(self, fgraph, node, input_shapes):
        return [(input_shapes[0][0],)]

    def perform(self, node, inputs, outputs):
        T, R, q, Z, d, Hdiag, shift = inputs
        out = batched.kalman_logp_segments_batched(T, R, q, Z, self.y, self.seg_start, Hdiag=Hdiag, d=d, shift=shift, outputs=("logp",),
                                                   **self._kwargs())
        outputs[0][0] = out["logp"]

    def pullback(self, inputs, outputs, cotangents):
        """Cotangents of T, R, q, Z, d, Hdiag, shift: the per-draw ones of the reverse sweep times the cotangent of logp; an input
        shared by the draws (no leading draw axis) receives the sum over the batch."""
        T, R, q, Z, d, Hdiag, shift = inputs
        g = cotangents[0]
        bars = HipKalmanLogpSegmentsGrad(self.y, self.seg_start, q_mode=self.q_mode, jitter=self.jitter,
                                         missing_fill_value=self.missing_fill_value,
                                         conventions=None if self.conventions is None else dict(self.conventions))(*inputs)
        out = []
        for x, bar in zip(inputs, bars):
            w = bar * g.reshape((-1,) + (1,) * (bar.type.ndim - 1))
            out.append(w.sum(axis=0) if x.type.ndim < bar.type.ndim else w)
        return out


class HipKalmanLogpSegmentsGrad(_SegmentsOp):
    """``T_bar, R_bar, q_bar, Z_bar, d_bar, h_bar, shift_bar = Op(T, R, q, Z, d, Hdiag, shift)`` per draw, for a unit cotangent of
    logp (``batched.kalman_logp_segments_grad_batched``): every output has the leading draw axis, also where its input is shared;
    q_bar is (batch, S, k) for a diagonal covariance and (batch, S, k, k), the symmetric convention, for a full one."""

    def make_node(self, T, R, q, Z, d, Hdiag, shift):
        _require()
        inputs = [pt.as_tensor(x) for x in (T, R, q, Z, d, Hdiag, shift)]
        T_ = inputs[0]
        b = T_.type.shape[:1]
        full = self._q_full(len(inputs[2].type.shape))
        outputs = []
        for x, name, nd in zip(inputs, ("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar"), (4, 4, 4 if full else 3, 4, 3, 3, 3)):
            shape = tuple(x.type.shape)
            outputs.append(pt.tensor(name, dtype="float64", shape=shape if len(shape) == nd else b + shape))
        return Apply(self, inputs, outputs)

    def _q_full(self, ndim):
        """Whether q is a full covariance: by ``q_mode``, else by its number of axes -- (S, k) and (batch, S, k, k) are unambiguous,
        three axes are (batch, S, k) or (S, k, k) and need ``q_mode``."""
        if self.q_mode is not None:
            return self.q_mode in ("full", "full_batched")
        if ndim == 3:
            raise ValueError("q with three axes is (batch, S, k) or (S, k, k): pass q_mode")
        return ndim == 4

    def infer_shape(self, fgraph, node, input_shapes):
        b = input_shapes[0][0]
        return [tuple(s) if len(s) == out.type.ndim else (b, *s) for s, out in zip(input_shapes, node.outputs)]

    def perform(self, node, inputs, outputs):
        T, R, q, Z, d, Hdiag, shift = inputs
        out = batched.kalman_logp_segments_grad_batched(T, R, q, Z, self.y, self.seg_start, Hdiag=Hdiag, d=d, shift=shift,
                                                        outputs=("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar"),
                                                        **self._kwargs())
        qb = out["Q_bar"] if "Q_bar" in out else out["q_bar"]
        for cell, val in zip(outputs, (out["T_bar"], out["R_bar"], qb, out["Z_bar"], out["d_bar"], out["h_bar"], out["shift_bar"])):
            cell[0] = val


class HipGensys(Op):
    """Drop-in for ``GensysWrapper`` (gEconpy/solvers/gensys.py:634-676): ``T, success = Op(A, B, C, D)``
    with ``__props__ = ("tol",)``, the same ``gufunc_signature``, ``T`` (n, n) of dtype floatX (as upstream) and a boolean
    scalar ``success = (eu[0] == 1 and eu[1] == 1)`` (:663).  Batched (leading draw axis) inputs give
    (batch, n, n) and (batch,) outputs from ONE launch.  ``pullback`` returns the adjoints of
    (A, B, C) from the cotangent of T on the device and a zero cotangent for D (:668-676)."""

    __props__ = ("tol",)
    gufunc_signature = "(n,n),(n,n),(n,n),(n,k)->(n,n),()"

    def __init__(self, tol=1e-8):
        self.tol = tol
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C, D):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C, D)]
        shp = inputs[0].type.shape
        # the reference declares T without a dtype, i.e. floatX (gensys.py:646); the kernels compute in float64 and
        # perform() casts to the declared type
        outputs = [pt.tensor("T", dtype=_floatx(), shape=shp), pt.tensor("success", dtype="bool", shape=shp[:-2])]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        return [input_shapes[0], input_shapes[0][:-2]]

    def perform(self, node, inputs, outputs):
        squeeze = np.ndim(inputs[0]) == 2
        A, B, C, D = (_as3(x) for x in inputs)
        if D.shape[:2] != A.shape[:2]:
            raise ValueError(f"D must be (n, k) with n = {A.shape[1]}; got {D.shape[1:]}")
        # T = G1[:n,:n] and eu do not depend on D (psi only enters `impact`, gensys.py:359-365): it is not shipped to the device
        out = batched.gensys_batched(A, B, C, None, tol=self.tol)
        T = out["T"][0] if squeeze else out["T"]
        dt = getattr(getattr(node.outputs[0], "type", None), "dtype", "float64") if node is not None else "float64"
        outputs[0][0] = np.asarray(T, dtype=dt)
        outputs[1][0] = np.asarray(out["success"][0] if squeeze else out["success"], dtype=bool)

    def pullback(self, inputs, outputs, cotangents):
        _A, B, C, D = inputs
        A_bar, B_bar, C_bar = HipPolicyAdjoint()(B, C, outputs[0], cotangents[0])
        return [A_bar, B_bar, C_bar, pt.zeros_like(D)]


def gensys_pt(A, B, C, D, tol=1e-8):
    """Same signature and return as ``gEconpy.solvers.gensys.gensys_pt`` (:679-683): ``(T, R, success)``."""
    T, success = HipGensys(tol=tol)(A, B, C, D)
    R = HipSelection()(B, C, D, T)
    return T, R, success


class HipBKEigenvalues(Op):
    """``real, imag, n_unstable = Op(A, B, C)``: the generalized eigenvalues of the Sims pencil sorted by modulus (what
    ``compute_bk_eigenvalues_pt`` returns through ``real_eig``, gEconpy/model/perturbation.py:448-505) and the number of
    them with modulus > 1, from ``dsge_bk_eigenvalues_batched``.  The reference's graph regularises Gamma_0 and takes a dense
    ``eig``; the counts -- all the BK condition uses -- are the same.  Not differentiable: the reference detaches the
    eigenvalues as well (``disconnected_grad``, :608-611)."""

    __props__ = ("tol", "n_forward")

    def __init__(self, n_forward, tol=1e-8):
        self.tol = tol
        self.n_forward = int(n_forward)
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C)]
        n = inputs[0].type.shape[-1]
        N = None if n is None else n + self.n_forward
        outputs = [pt.tensor("eig_real", dtype="float64", shape=(N,)), pt.tensor("eig_imag", dtype="float64", shape=(N,)),
                   pt.tensor("n_unstable", dtype="int64", shape=())]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        N = input_shapes[0][-1] + self.n_forward
        return [(N,), (N,), ()]

    def perform(self, node, inputs, outputs):
        A, B, C = (_as3(x) for x in inputs)
        out = batched.bk_eigenvalues_batched(A, B, C, tol=self.tol)
        m = int(out["n_eig"][0])
        outputs[0][0] = out["real"][0, :m].copy()
        outputs[1][0] = out["imag"][0, :m].copy()
        outputs[2][0] = np.asarray(out["n_unstable"][0], dtype=np.int64)


def check_bk_condition_pt(A, B, C, D, lead_var_idx, tol=1e-8):
    """Same signature and return as ``gEconpy.model.perturbation.check_bk_condition_pt`` (:586-625):
    ``(bk_satisfied, n_forward, n_unstable)``; ``D`` is unused there too."""
    n_forward = len(np.asarray(lead_var_idx))
    _re, _im, n_unstable = HipBKEigenvalues(n_forward, tol=tol)(A, B, C)
    return pt.eq(n_forward, n_unstable), pt.constant(n_forward), n_unstable


class HipScanCycleReduction(Op):
    """``T, n_steps = Op(A, B, C)`` with the semantics of ``_scan_cycle_reduction``
    (gEconpy/solvers/cycle_reduction.py:246-294): fixed trip count, A0-norm-only stopping rule, 1e-16
    diagonal jitter.  (n, n) or (batch, n, n) inputs."""

    __props__ = ("max_iter", "tol")
    gufunc_signature = "(n,n),(n,n),(n,n)->(n,n),()"

    def __init__(self, max_iter=50, tol=1e-7):
        self.max_iter = int(max_iter)
        self.tol = tol
        if _HAVE_PYTENSOR:
            super().__init__()

    def make_node(self, A, B, C):
        _require()
        inputs = [pt.as_tensor(x) for x in (A, B, C)]
        shp = inputs[0].type.shape
        outputs = [pt.tensor("T", dtype="float64", shape=shp), pt.tensor("n_steps", dtype="int32", shape=shp[:-2])]
        return Apply(self, inputs, outputs)

    def infer_shape(self, fgraph, node, input_shapes):
        return [input_shapes[0], input_shapes[0][:-2]]

    def perform(self, node, inputs, outputs):
        squeeze = np.ndim(inputs[0]) == 2
        A, B, C = (_as3(x) for x in inputs)
        T, _status, n_steps = batched.scan_cycle_reduction_batched(A, B, C, max_iter=self.max_iter, tol=self.tol)
        outputs[0][0] = T[0] if squeeze else T
        outputs[1][0] = np.asarray(n_steps[0] if squeeze else n_steps, dtype=np.int32)

    def pullback(self, inputs, outputs, cotangents):
        _A, B, C = inputs
        return list(HipPolicyAdjoint()(B, C, outputs[0], cotangents[0]))


def scan_cycle_reduction(A, B, C, D, max_iter=50, tol=1e-7, mode=None, use_adjoint_gradients=True):
    """Same signature and return as ``gEconpy.solvers.cycle_reduction.scan_cycle_reduction`` (:297-325):
    ``(T, R, n_steps)``.  ``mode`` is accepted for signature compatibility (there is no scan to compile);
    gradients always use the adjoint solve."""
    del mode, use_adjoint_gradients
    T, n_steps = HipScanCycleReduction(max_iter=max_iter, tol=tol)(A, B, C)
    R = HipSelection()(B, C, D, T)
    return T, R, n_steps


def cycle_reduction_pt(A, B, C, D, max_iter=1000, tol=1e-9):
    """Same signature and return as ``gEconpy.solvers.cycle_reduction.cycle_reduction_pt``
    (:216-219): ``(T, R)``."""
    T = HipCycleReduction(max_iter=max_iter, tol=tol)(A, B, C)
    R = HipSelection()(B, C, D, T)
    return T, R


def _register_vectorize():
    """Teach pytensor to vectorise the per-draw Ops into ONE batched launch instead of a Blockwise loop over draws."""
    try:
        from pytensor.graph.replace import _vectorize_node  # noqa: PLC0415
    except Exception:  # noqa: BLE001
        return False

    @_vectorize_node.register(HipCycleReduction)
    def _vectorize_hip_cr(op, node, A, B, C):
        if A.type.ndim == 3 and B.type.ndim == 3 and C.type.ndim == 3:
            return HipCycleReductionBatched(max_iter=op.max_iter, tol=op.tol).make_node(A, B, C)
        from pytensor.tensor.blockwise import Blockwise  # noqa: PLC0415

        return Blockwise(op).make_node(A, B, C)

    def _native(op_cls):  # Ops whose perform already takes a leading draw axis on every input
        @_vectorize_node.register(op_cls)
        def _vec(op, node, *batched_inputs):
            nd = {x.type.ndim for x in batched_inputs}
            if nd == {3}:
                return op.make_node(*batched_inputs)
            from pytensor.tensor.blockwise import Blockwise  # noqa: PLC0415

            return Blockwise(op).make_node(*batched_inputs)

    for cls in (HipGensys, HipSelection, HipSelectionAdjoint, HipPolicyAdjoint, HipScanCycleReduction):
        _native(cls)
    return True


# ---- backend dispatch: numba and JAX (gensys.py:686-713, cycle_reduction.py:222-243, real_eig.py:100-137) ------------------
def make_numba_cycle_reduction(njit, cr_host, max_iter, tol, out_dtype=np.float64):
    """The njit-compiled twin of ``HipCycleReduction.perform``: numba calls the SAME C entry point
    (``dsge_cycle_reduction_batched_host``, batch = 1) through its ctypes binding, so the numba backend neither falls
    back to object mode nor to a CPU solver.  ``njit`` is the decorator (pytensor's ``numba_njit`` or ``numba.njit``);
    ``cr_host`` the ctypes function.  A malformed call / missing device gives a NaN matrix (numba code cannot raise
    the library's error message)."""
    max_iter = int(max_iter)
    tol = float(tol)

    @njit
    def cycle_reduction(A, B, C):
        n = A.shape[0]
        A64 = np.ascontiguousarray(A).astype(np.float64)
        B64 = np.ascontiguousarray(B).astype(np.float64)
        C64 = np.ascontiguousarray(C).astype(np.float64)
        T = np.zeros((n, n), dtype=np.float64)
        status = np.zeros(1, dtype=np.int32)
        n_iter = np.zeros(1, dtype=np.int32)
        rc = cr_host(A64.ctypes, B64.ctypes, C64.ctypes, 1, n, max_iter, tol, T.ctypes, status.ctypes, n_iter.ctypes)
        if rc != 0:
            T[:, :] = np.nan
        return T.astype(out_dtype)

    return cycle_reduction


def make_numba_gensys(njit, gensys_host, tol):
    """njit twin of ``HipGensys.perform`` -> ``(T, success)`` through ``dsge_gensys_batched_host`` (batch = 1)."""
    tol = float(tol)

    @njit
    def gensys_wrapper(A, B, C, D):
        n = A.shape[0]
        A64 = np.ascontiguousarray(A).astype(np.float64)
        B64 = np.ascontiguousarray(B).astype(np.float64)
        C64 = np.ascontiguousarray(C).astype(np.float64)
        D64 = np.ascontiguousarray(D).astype(np.float64)
        k = D64.shape[1]
        T = np.zeros((n, n), dtype=np.float64)
        R = np.zeros((n, k), dtype=np.float64)  # (real buffers for D and R: numba may refuse to type an integer 0 as a pointer)
        eu = np.zeros(3, dtype=np.int32)
        status = np.ones(1, dtype=np.int32)
        rc = gensys_host(A64.ctypes, B64.ctypes, C64.ctypes, D64.ctypes, 1, n, k, tol, 0, T.ctypes, R.ctypes, eu.ctypes,
                         status.ctypes)
        success = (rc == 0) and (eu[0] == 1) and (eu[1] == 1)
        return T, success

    return gensys_wrapper


def _register_numba():
    try:
        from pytensor.link.numba.dispatch import basic as numba_basic  # noqa: PLC0415
        from pytensor.link.numba.dispatch.basic import register_funcify_default_op_cache_key  # noqa: PLC0415
    except Exception:  # noqa: BLE001
        return False
    from . import _lib  # noqa: PLC0415

    @register_funcify_default_op_cache_key(HipCycleReduction)
    def numba_funcify_HipCycleReduction(op, node, **kwargs):  # noqa: ARG001
        fn = make_numba_cycle_reduction(numba_basic.numba_njit, _lib.load().dsge_cycle_reduction_batched_host, op.max_iter,
                                        op.tol, node.outputs[0].type.numpy_dtype)
        # no cache key: the compiled function holds the ADDRESS of a ctypes function of this process's library; an on-disk
        # cache entry would outlive it
        return fn, None

    @register_funcify_default_op_cache_key(HipGensys)
    def numba_funcify_HipGensys(op, node, **kwargs):  # noqa: ARG001
        fn = make_numba_gensys(numba_basic.numba_njit, _lib.load().dsge_gensys_batched_host, op.tol)
        return fn, None

    return True


def _register_jax():
    """JAX backend: the Ops run as host callbacks (``jax.pure_callback``) into the same ``perform`` -- the library owns
    its own device buffers, JAX only sees numpy in / numpy out with the shapes ``infer_shape`` gives."""
    try:
        import jax  # noqa: PLC0415
        from pytensor.link.jax.dispatch.basic import jax_funcify  # noqa: PLC0415
    except Exception:  # noqa: BLE001
        return False

    def _callback(op, node):
        def fn(*inputs):
            shapes = [jax.ShapeDtypeStruct(tuple(int(d) for d in s), np.dtype(o.type.dtype))
                      for s, o in zip(op.infer_shape(None, node, [tuple(x.shape) for x in inputs]), node.outputs)]

            def host(*arrays):
                cells = [[None] for _ in node.outputs]
                op.perform(node, [np.asarray(a) for a in arrays], cells)
                return tuple(np.asarray(c[0], dtype=sd.dtype).reshape(sd.shape) for c, sd in zip(cells, shapes))

            try:  # batched by running the callback once per element (the library call is itself batched where it matters)
                res = jax.pure_callback(host, tuple(shapes), *inputs, vmap_method="sequential")
            except TypeError:  # older jax: no vmap_method keyword
                res = jax.pure_callback(host, tuple(shapes), *inputs)
            return res[0] if len(res) == 1 else res

        return fn

    for cls in (HipCycleReduction, HipGensys, HipSelection, HipSelectionAdjoint, HipPolicyAdjoint, HipScanCycleReduction,
                HipCycleReductionBatched, HipSolveKalmanLogp, HipSolveKalmanLogpGrad, HipBKEigenvalues):
        jax_funcify.register(cls)(lambda op, node, **kwargs: _callback(op, node))  # noqa: ARG005
    return True


if _HAVE_PYTENSOR:  # registration by import side effect
    _register_vectorize()
    _register_numba()
    _register_jax()
