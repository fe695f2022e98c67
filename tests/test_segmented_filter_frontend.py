"""CPU: the front end of the Kalman likelihood across dated breaks (``_frontend.kalman_logp_segments`` and the fused
``solve_kalman_logp_segments``) reads every layout off the shapes, refuses a malformed list of breaks before the library is called, and
the library -- device entry and host twin -- refuses the same before any device is touched (this machine may have none).  The kernels of
the entry use no scratch memory."""
import os
import re

import numpy as np
import pytest

from geconpy_amd import _lib, batched

NB, S, M, K, P, N = 2, 3, 5, 2, 2, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = (0, 3, 6)


def _model(nb=NB, s=S, m=M, k=K):
    return np.zeros((nb, s, m, m)), np.zeros((nb, s, m, k))


def _rest(s=S, m=M, k=K, p=P, n=N):
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


def test_max_segments_matches_the_header_and_the_abi_version_is_unchanged():
    text = open(os.path.join(ROOT, "include", "dsge_hip.h")).read()
    consts = dict(re.findall(r"#define\s+(DSGE_[A-Z_0-9]+)\s+(-?\d+)", text))
    assert int(consts["DSGE_MAX_SEGMENTS"]) == _lib.MAX_SEGMENTS == 8
    assert int(consts["DSGE_ABI_VERSION"]) == _lib.ABI_VERSION == 19
    sig = [a for a, _ in _lib.SIGNATURES["dsge_kalman_logp_segments_batched"]]
    assert sig[sig.index("a0"):sig.index("batch")] == ["a0", "P0", "shift", "y", "seg_start", "n_seg"]
    assert sig[-6:] == ["logp_out", "ll_out", "a_last_out", "P_last_out", "status_io", "stream"]
    assert [a for a, _ in _lib.SIGNATURES["dsge_kalman_logp_segments_batched_host"]] == sig[:-1]


def test_every_layout_is_read_off_the_shapes(recorded):
    call = batched.kalman_logp_segments_batched
    T, R = _model()
    q, Z, y = _rest()
    r = call(T, R, q, Z, y, SEG)
    a = recorded.named
    assert recorded.entry == "dsge_kalman_logp_segments_batched"
    assert (a["batch"], a["n_seg"], a["m"], a["k"], a["p"], a["T_len"]) == (NB, S, M, K, P, N)
    assert (a["q_mode"], a["z_batched"], a["d_batched"], a["h_batched"]) == (_lib.Q_DIAG_SHARED, 0, 0, 0)
    assert all(a[key] is None for key in ("d", "Hdiag", "a0", "P0", "shift"))
    assert isinstance(a["seg_start"], int) and a["seg_start"] != 0  # (a host address, for the device front end too)
    assert sorted(r) == ["P_last", "a_last", "ll", "logp", "status"]
    assert r["logp"].shape == (NB,) and r["ll"].shape == (NB, N) and r["a_last"].shape == (NB, M) and r["P_last"].shape == (NB, M, M)
    assert r["status"].dtype == np.int32 and not r["status"].any()
    for qq, code in ((np.ones((NB, S, K)), _lib.Q_DIAG_BATCHED), (np.ones((S, K, K)), _lib.Q_FULL_SHARED),
                     (np.ones((NB, S, K, K)), _lib.Q_FULL_BATCHED)):
        call(T, R, qq, Z, y, SEG)
        assert recorded.named["q_mode"] == code
    call(T, R, q, np.zeros((NB, S, P, M)), y, SEG, d=np.zeros((NB, S, P)), Hdiag=np.zeros((S, P)), a0=np.zeros((NB, M)),
         P0=np.zeros((NB, M, M)), shift=np.zeros((NB, S, M)), jitter=0.5, missing_fill_value=-1.0)
    a = recorded.named
    assert (a["z_batched"], a["d_batched"], a["h_batched"], a["jitter"], a["missing_fill"]) == (1, 1, 0, 0.5, -1.0)
    assert all(a[key] is not None for key in ("d", "Hdiag", "a0", "P0", "shift"))
    r = call(T, R, q, Z, y, SEG, outputs=("logp",))
    a = recorded.named
    assert a["logp_out"] is not None and a["ll_out"] is None and a["a_last_out"] is None and a["P_last_out"] is None
    assert r["ll"] is None and r["a_last"] is None and r["P_last"] is None
    r = call(T, R, q, Z, y, SEG, outputs=("P_last",))
    assert recorded.named["P_last_out"] is not None and recorded.named["ll_out"] is None and r["logp"] is not None
    # S = 1 and S = 8; a list, a tuple or an array of any integer type
    call(*_model(s=1), *_rest(s=1), [0])
    assert recorded.named["n_seg"] == 1
    call(*_model(s=8), *_rest(s=8), np.arange(8, dtype=np.int64))
    assert recorded.named["n_seg"] == 8


def test_the_fused_front_end_flattens_solves_and_filters(recorded):
    A = np.zeros((NB, S, M, M))
    D = np.zeros((NB, S, M, K))
    q, Z, y = _rest()
    for solver, first in (("cycle_reduction", ["dsge_cycle_reduction_batched", "dsge_selection_batched"]),
                          ("gensys", ["dsge_gensys_batched"]), ("backward_direct", ["dsge_backward_direct_batched"])):
        recorded.entries.clear()
        r = batched.solve_kalman_logp_segments_batched(A, A, A, D, q, Z, y, SEG, solver=solver)
        assert recorded.entries == first + ["dsge_kalman_logp_segments_batched"]
        assert r["T"].shape == (NB, S, M, M) and r["R"].shape == (NB, S, M, K) and r["status"].shape == (NB,)
        assert (recorded.named["batch"], recorded.named["n_seg"], recorded.named["m"], recorded.named["k"]) == (NB, S, M, K)


def test_every_refusal_comes_before_the_library_is_called(no_library):
    T, R = _model()
    q, Z, y = _rest()
    A, D = np.zeros((NB, S, M, M)), np.zeros((NB, S, M, K))
    for call, head in ((batched.kalman_logp_segments_batched, (T, R)), (batched.solve_kalman_logp_segments_batched, (A, A, A, D))):
        with pytest.raises(ValueError, match="1 .. 8 segments"):
            call(*head, q, Z, y, ())
        with pytest.raises(ValueError, match="1 .. 8 segments"):
            call(*head, q, Z, np.zeros((12, P)), tuple(range(9)))
        with pytest.raises(ValueError, match=r"seg_start\[0\] must be 0"):
            call(*head, q, Z, y, (1, 3, 6))
        with pytest.raises(ValueError, match="strictly increasing"):
            call(*head, q, Z, y, (0, 3, 3))
        with pytest.raises(ValueError, match="strictly increasing"):
            call(*head, q, Z, y, (0, 5, 4))
        with pytest.raises(ValueError, match="< T_len = 8"):
            call(*head, q, Z, y, (0, 3, 8))
        with pytest.raises(ValueError, match="required"):
            call(*head, q, Z, y, None)
        with pytest.raises(ValueError, match="integers"):
            call(*head, q, Z, y, (0, 2.5, 6))
        with pytest.raises(ValueError, match="required"):
            call(*head, q, None, y, SEG)
        with pytest.raises(ValueError, match="required"):
            call(*head, q, Z, None, SEG)
        with pytest.raises(ValueError, match="required"):
            call(head[0], None, *head[2:], q, Z, y, SEG)
    call = batched.kalman_logp_segments_batched
    with pytest.raises(ValueError, match="2 entries, T has 3 segments"):
        call(T, R, q, Z, y, (0, 3))
    with pytest.raises(ValueError, match="cannot infer the layout of Q"):
        call(T, R, np.ones((S + 1, K)), Z, y, SEG)
    with pytest.raises(ValueError, match="Z must be"):
        call(T, R, q, np.zeros((P, M)), y, SEG)
    with pytest.raises(ValueError, match="d must be"):
        call(T, R, q, Z, y, SEG, d=np.zeros(P))
    with pytest.raises(ValueError, match="Hdiag must be"):
        call(T, R, q, Z, y, SEG, Hdiag=np.zeros((NB, P)))
    with pytest.raises(ValueError, match="a0 must be"):
        call(T, R, q, Z, y, SEG, a0=np.zeros(M))
    with pytest.raises(ValueError, match="P0 must be"):
        call(T, R, q, Z, y, SEG, P0=np.zeros((NB, M)))
    with pytest.raises(ValueError, match="shift must be"):
        call(T, R, q, Z, y, SEG, shift=np.zeros((NB, M)))
    with pytest.raises(ValueError, match="outputs must be among"):
        call(T, R, q, Z, y, SEG, outputs=("logp", "a_pred"))
    with pytest.raises(ValueError, match="T must be"):
        call(T[:, :, :4], R, q, Z, y, SEG)
    with pytest.raises(ValueError, match="solver must be"):
        batched.solve_kalman_logp_segments_batched(A, A, A, D, q, Z, y, SEG, solver="scan_cycle_reduction")


def _c_args(T, R, q, Z, y, seg, n_seg, *, m=M, k=K, p=P, T_len=N, batch=NB, logp=True, status=True, q_mode=0):
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    lp, st = np.zeros(NB), np.zeros(NB, dtype=np.int32)
    keep = (lp, st)
    return keep, [ptr(T), ptr(R), ptr(q), q_mode, ptr(Z), 0, None, 0, None, 0, None, None, None, ptr(y), ptr(seg), n_seg, batch, m, k, p,
                  T_len, 1e-8, -9999.0, ptr(lp) if logp else None, None, None, None, ptr(st) if status else None]


@pytest.mark.parametrize("entry", ("dsge_kalman_logp_segments_batched", "dsge_kalman_logp_segments_batched_host"))
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
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, logp=False) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, status=False) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, q_mode=4) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, k=M + 1) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, batch=-1) == _lib.ERR_INVALID
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, m=_lib.MAX_N + 1) == _lib.ERR_TOO_LARGE
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, p=_lib.MAX_P + 1) == _lib.ERR_TOO_LARGE
    # with T_len == 0 the list is not held against the panel
    assert rc(T, R, q, Z, y, i32(0, 3, 6), 3, T_len=0) != _lib.ERR_INVALID


def test_no_kernel_of_the_entry_uses_scratch_memory(tmp_path):
    """The measurement update solves K row by row inside LDS and the list of breaks is read with constant indices out of the kernel
    arguments: neither may turn into a private array (scratch) unnoticed."""
    import subprocess

    from geconpy_amd import build

    out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "a.o"),
                          os.path.join(build.CSRC, "launch_kalman_seg.hip")], cwd=build.CSRC, capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S*kernel\S*)", out.stderr)
    sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len({n for n in names if "kalman_seg_kernel" in n}) == 1 and len({n for n in names if "kseg_rows_kernel" in n}) == 1
    assert len(sizes) >= 2 and set(sizes) == {"0"}
