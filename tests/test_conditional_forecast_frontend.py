"""CPU: the front end of the conditional forecast (``_frontend.conditional_forecast``) refuses what is malformed before any call and
turns its inputs into the layouts of the C ABI, and the library refuses what is too large or malformed before any device is
touched (this machine may have none)."""
import numpy as np
import pytest

from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

NB, M, K, P, STEPS = 2, 6, 3, 2, 5


def _inputs(nb=NB, m=M, k=K):
    return np.zeros((nb, m, m)), np.zeros((nb, m, k)), np.ones(k), np.zeros((nb, m))


def _conds(pairs, steps=STEPS, p=P, lead=()):
    c = np.full((*lead, steps, p), np.nan)
    for t, j in pairs:
        c[..., t, j] = 0.1
    return c


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _NoCall())


class _Recorder:
    """Stands in for ``_lib.call``: keeps the named arguments of the one call."""

    def __call__(self, entry, *, host, stream=None, **named):
        self.entry, self.named = entry, named


@pytest.fixture
def recorded(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def test_the_nan_pattern_becomes_ascending_pairs():
    c = _conds([(3, 0), (0, 1), (1, 0), (1, 1)])
    c[1, 1] = 0.7
    ct, cj, vals = F.condition_pattern(c, NB, 1, P, STEPS)
    assert ct.tolist() == [0, 1, 1, 3] and cj.tolist() == [1, 0, 1, 0] and ct.dtype == cj.dtype == np.int32
    assert vals.tolist() == [0.1, 0.1, 0.7, 0.1]
    ct, cj, vals = F.condition_pattern(_conds([(2, 1)], lead=(NB, 4)), NB, 4, P, STEPS)
    assert ct.tolist() == [2] and cj.tolist() == [1] and vals.shape == (NB, 4, 1)
    ct, cj, vals = F.condition_pattern(_conds([]), NB, 1, P, STEPS)
    assert len(ct) == 0 and vals.shape == (0,)
    ct, cj, vals = F.condition_pattern(([0, 2], [1, 0], np.zeros((NB, 2))), NB, 1, P, STEPS)
    assert ct.tolist() == [0, 2] and cj.tolist() == [1, 0]


def test_a_nan_pattern_that_differs_between_draws_or_paths_is_a_value_error(no_library):
    T, R, Q, x0 = _inputs()
    c = _conds([(0, 0), (1, 1)], lead=(NB,))
    c[1, 1, 1] = np.nan
    with pytest.raises(ValueError, match="NaN pattern"):
        batched.conditional_forecast_batched(T, R, Q, x0, c, STEPS, Z=np.eye(P, M))
    c = _conds([(0, 0)], lead=(NB, 3))
    c[0, 2, 4, 1] = 0.0
    with pytest.raises(ValueError, match="NaN pattern"):
        batched.conditional_forecast_batched(T, R, Q, x0, c, STEPS, Z=np.eye(P, M))


def test_shape_mismatches_are_value_errors(no_library):
    T, R, Q, x0 = _inputs()
    Z, c = np.eye(P, M), _conds([(0, 0)])
    call = batched.conditional_forecast_batched
    with pytest.raises(ValueError, match="Z is required"):
        call(T, R, Q, x0, c, STEPS)
    with pytest.raises(ValueError, match="Z must be"):
        call(T, R, Q, x0, c, STEPS, Z=np.eye(P, M + 1))
    with pytest.raises(ValueError, match="conditions must be"):
        call(T, R, Q, x0, _conds([(0, 0)], p=P + 1), STEPS, Z=Z)
    with pytest.raises(ValueError, match="leading axes"):
        call(T, R, Q, x0, _conds([(0, 0)], lead=(NB + 1,)), STEPS, Z=Z)
    with pytest.raises(ValueError, match="periods"):
        call(T, R, Q, x0, _conds([(0, 0)], steps=STEPS + 1), STEPS, Z=Z)
    with pytest.raises(ValueError, match="n_steps"):
        call(T, R, Q, x0, c, 0, Z=Z)
    with pytest.raises(ValueError, match="x0 must be"):
        call(T, R, Q, np.zeros((NB, M + 1)), c, STEPS, Z=Z)
    with pytest.raises(ValueError, match="x0 must be"):
        call(T, R, Q, np.zeros((NB + 1, M)), c, STEPS, Z=Z)
    with pytest.raises(ValueError, match="eps must be"):
        call(T, R, Q, x0, c, STEPS, Z=Z, eps=np.zeros((4, STEPS, K + 1)))
    with pytest.raises(ValueError, match="shock steps"):
        call(T, R, Q, x0, c, STEPS, Z=Z, eps=np.zeros((4, STEPS + 1, K)))
    with pytest.raises(ValueError, match="agree"):
        call(T, R, Q, x0, c, STEPS, Z=Z, eps=np.zeros((4, STEPS, K)), n_paths=3)
    with pytest.raises(ValueError, match="agree"):
        call(T, R, Q, np.zeros((NB, 5, M)), _conds([(0, 0)], lead=(NB, 4)), STEPS, Z=Z)
    with pytest.raises(ValueError, match="free_shocks"):
        call(T, R, Q, x0, c, STEPS, Z=Z, free_shocks=[0, K])
    with pytest.raises(ValueError, match="free_shocks"):
        call(T, R, Q, x0, c, STEPS, Z=Z, free_shocks=np.array([True, False]))
    with pytest.raises(ValueError, match="status"):
        call(T, R, Q, x0, c, STEPS, Z=Z, status=np.zeros(NB + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="Q"):
        call(T, R, np.ones(K + 1), x0, c, STEPS, Z=Z)
    with pytest.raises(ValueError, match="at most 96"):
        call(*_inputs(m=97), c, STEPS, Z=np.eye(P, 97))


def test_shapes_become_the_flags_of_the_abi(recorded):
    T, R, Q, x0 = _inputs()
    Z = np.eye(P, M)
    r = batched.conditional_forecast_batched(T, R, Q, x0, _conds([(0, 1), (2, 0)]), STEPS, Z=Z, free_shocks=[2, 0])
    a = recorded.named
    assert recorded.entry == "dsge_conditional_forecast_batched"
    assert (a["n_cond"], a["cv_batched"], a["cv_paths"], a["x0_batched"], a["x0_paths"], a["n_paths"], a["n_shock_steps"]) == (2, 0, 0, 1, 0, 1, 0)
    assert a["eps"] is None and a["d"] is None and a["q_mode"] == _lib.Q_DIAG_SHARED and a["rank_tol"] == 0.0
    assert r["x"].shape == (NB, 1, STEPS, M) and r["shocks"].shape == (NB, 1, STEPS, K) and r["observed"].shape == (NB, 1, STEPS, P)
    assert r["status"].shape == (NB,) and r["status"].dtype == np.int32
    r = batched.conditional_forecast_batched(T, R, np.ones((NB, K, K)), np.zeros((1, 4, M)), _conds([(1, 1)], lead=(NB,)), STEPS, Z=Z,
                                             d=np.zeros((NB, P)), eps=np.zeros((NB, 4, 3, K)), free_shocks=np.array([True, False, True]))
    a = recorded.named
    assert (a["n_cond"], a["cv_batched"], a["cv_paths"], a["x0_batched"], a["x0_paths"], a["n_paths"], a["n_shock_steps"]) == (1, 1, 0, 0, 1, 4, 3)
    assert (a["eps_batched"], a["d_batched"], a["z_batched"], a["q_mode"]) == (1, 1, 0, _lib.Q_FULL_BATCHED)
    assert r["x"].shape == (NB, 4, STEPS, M)
    batched.conditional_forecast_batched(T, R, Q, np.zeros(M), _conds([(1, 1)], lead=(NB, 3)), STEPS, Z=Z, eps=np.zeros((3, 2, K)))
    a = recorded.named
    assert (a["cv_batched"], a["cv_paths"], a["x0_batched"], a["x0_paths"], a["n_paths"], a["eps_batched"]) == (1, 1, 0, 0, 3, 0)
    batched.conditional_forecast_batched(T, R, Q, x0, _conds([]), STEPS, Z=Z, n_paths=2)  # no condition: the unconditional path
    assert recorded.named["n_cond"] == 0 and recorded.named["cond_t"] is None and recorded.named["n_paths"] == 2


def _raw(T, R, Q, x0, *, pairs=((0, 0),), Z="eye", p=P, n_steps=STEPS, n_paths=1, free=None, eps=None, n_shock=0, q_mode=0,
         vals="zeros", outs=(True, True, True)):
    """The host twin called directly: the return code, with everything after the refusal never reached on a machine without a GPU."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nb, m, k = (NB, M, K) if R is None else R.shape
    Z = np.eye(p, m) if isinstance(Z, str) else Z
    ct, cj = (np.array([pr[i] for pr in pairs], dtype=np.int32) for i in (0, 1))
    vals = np.zeros(max(len(pairs), 1)) if isinstance(vals, str) else vals
    fr = None if free is None else np.ascontiguousarray(free, dtype=np.int32)
    x, e, o = (np.empty((nb, n_paths, max(n_steps, 1), w)) if on else None for w, on in zip((m, k, max(p, 1)), outs))
    return lib.dsge_conditional_forecast_batched_host(ptr(T), ptr(R), ptr(Q), q_mode, ptr(Z), 0, None, 0, ptr(x0), 1, 0, ptr(eps), 0,
                                                      ptr(ct), ptr(cj), len(pairs), ptr(vals), 0, 0, ptr(fr), None, nb, m, k, p, n_paths,
                                                      n_steps, n_shock, 0.0, ptr(x), ptr(e), ptr(o))


def test_the_library_refuses_sizes_before_any_device():
    big = _lib.ERR_TOO_LARGE
    assert _raw(*_inputs(m=97)) == big
    assert b"DSGE_MAX_N_BIG" in _lib.load().dsge_last_error()
    assert _raw(*_inputs(m=20), p=17) == big
    assert b"DSGE_MAX_P" in _lib.load().dsge_last_error()
    pairs65 = [(t, j) for t in range(33) for j in (0, 1)][:65]
    assert _raw(*_inputs(), pairs=pairs65, n_steps=40) == big
    assert b"64 conditions" in _lib.load().dsge_last_error()
    # the LDS image: m = 96, k = 8 carries 36 conditions over 12 periods, not 64 conditions over 32 periods of all 8 shocks
    ok_pairs = [(t, j) for t in range(12) for j in (0, 1, 2)]
    assert _raw(*_inputs(m=96, k=8), pairs=ok_pairs, p=7, n_steps=12) in (0, _lib.ERR_HIP)  # (accepted: it goes on to the device)
    assert _raw(*_inputs(m=96, k=8), pairs=pairs65[:64], p=7, n_steps=40) == big
    assert b"160 KB" in _lib.load().dsge_last_error()
    # what the entry must carry at least is not refused: m = 64 with k = 16, n_cond = 64 with (t_max + 1) |F| = 256
    assert _raw(*_inputs(m=64, k=16), pairs=[(t, j) for t in range(16) for j in range(4)], p=16, n_steps=16) in (0, _lib.ERR_HIP)
    with pytest.raises(_lib.DsgeTooLargeError, match="64 conditions"):
        batched.conditional_forecast_batched(*_inputs(), _conds(pairs65, steps=40), 40, Z=np.eye(P, M))


def test_the_library_refuses_malformed_calls_before_any_device():
    bad = _lib.ERR_INVALID
    T, R, Q, x0 = _inputs()
    err = lambda: _lib.load().dsge_last_error()  # noqa: E731
    assert _raw(T, R, Q, x0, pairs=[(1, 0), (0, 1)]) == bad and b"ascending" in err()  # unsorted in t
    assert _raw(T, R, Q, x0, pairs=[(1, 1), (1, 0)]) == bad and b"ascending" in err()  # unsorted in j
    assert _raw(T, R, Q, x0, pairs=[(1, 1), (1, 1)]) == bad and b"ascending" in err()  # a pair twice
    assert _raw(T, R, Q, x0, pairs=[(STEPS, 0)]) == bad and b"cond_t" in err()
    assert _raw(T, R, Q, x0, pairs=[(-1, 0)]) == bad
    assert _raw(T, R, Q, x0, pairs=[(0, P)]) == bad and b"cond_j" in err()
    assert _raw(T, R, Q, x0, pairs=[(0, -1)]) == bad
    assert _raw(T, R, Q, x0, free=[0, 0, 0]) == bad and b"no free shock" in err()
    assert _raw(T, R, Q, x0, pairs=(), free=[0, 0, 0]) in (0, _lib.ERR_HIP)  # no condition needs no free shock
    assert _raw(T, R, Q, x0, n_steps=0, pairs=()) == bad and b"n_steps" in err()
    assert _raw(T, R, Q, x0, n_paths=0) == bad
    assert _raw(None, R, Q, x0) == bad and _raw(T, None, Q, x0) == bad and _raw(T, R, None, x0) == bad and _raw(T, R, Q, None) == bad
    assert _raw(T, R, Q, x0, Z=None) == bad
    assert _raw(T, R, Q, x0, vals=None) == bad  # conditions without values
    assert _raw(T, R, Q, x0, outs=(False, False, False)) == bad and b"no output" in err()
    assert _raw(T, R, Q, x0, outs=(False, True, False)) in (0, _lib.ERR_HIP)  # any one output is enough
    assert _raw(T, R, Q, x0, eps=np.zeros((NB, 1, STEPS + 1, K)), n_shock=STEPS + 1) == bad
    assert _raw(T, R, Q, x0, q_mode=4) == bad
    assert _raw(*_inputs(m=3, k=4)) == bad
    with pytest.raises(_lib.DsgeHipError, match="no free shock"):
        batched.conditional_forecast_batched(T, R, Q, x0, _conds([(0, 0)]), STEPS, Z=np.eye(P, M), free_shocks=[])


def test_the_abi_names_the_entry():
    assert _lib.ABI_VERSION >= 15
    assert _lib.ST_COND_SINGULAR == 512
    sig = [name for name, _ in _lib.SIGNATURES["dsge_conditional_forecast_batched"]]
    assert sig[-1] == "stream" and [name for name, _ in _lib.SIGNATURES["dsge_conditional_forecast_batched_host"]] == sig[:-1]
    assert "dsge_debug_condfc_phases" in _lib.SIGNATURES
