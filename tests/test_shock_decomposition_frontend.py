"""CPU: the front end of the historical shock decomposition (``_frontend.shock_decomposition``) refuses what is malformed before
any call, and the library refuses what is too large or malformed before any device is touched (this machine may have none)."""
import numpy as np
import pytest

from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

NB, M, K, T_LEN = 2, 6, 3, 4


def _inputs(nb=NB, m=M, k=K, T_len=T_LEN, n_paths=None):
    lead = (nb, T_len) if n_paths is None else (nb, n_paths, T_len)
    return np.zeros((nb, m, m)), np.zeros((nb, m, k)), np.zeros((*lead, m)), np.zeros((*lead, k))


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", _NoCall())


def test_groups_become_the_group_of_every_shock():
    of, g = F.shock_groups(None, 4)
    assert of.tolist() == [0, 1, 2, 3] and g == 4 and of.dtype == np.int32
    of, g = F.shock_groups([[3, 0], (1,), np.array([2])], 4)
    assert of.tolist() == [0, 1, 2, 0] and g == 3


@pytest.mark.parametrize("groups, match", [
    ([[0, 1]], "in no group"),
    ([[0, 1], [1, 2]], "shock 1 is in"),
    ([[0, 1, 2], []], "is empty"),
    ([[0, 1], [3]], "shock indices are"),
    ([[0, 1], [-1, 2]], "shock indices are"),
    ([0, 1, 2], "sequence of sequences"),
])
def test_a_bad_partition_is_a_value_error(no_library, groups, match):
    with pytest.raises(ValueError, match=match):
        batched.shock_decomposition_batched(*_inputs(), groups=groups)


def test_shape_mismatches_are_value_errors(no_library):
    T, R, x, e = _inputs()
    for bad in (dict(states=x[:, :, :5]), dict(shocks=e[:, :3]), dict(shocks=e[:, :, :2]), dict(states=x[:1], shocks=e[:1]),
                dict(states=x[0], shocks=e[0]), dict(states=x[:, None], shocks=e), dict(states=x[:, :0], shocks=e[:, :0])):
        with pytest.raises(ValueError):
            batched.shock_decomposition_batched(T, R, bad.get("states", x), bad.get("shocks", e))
    with pytest.raises(ValueError, match="Z must be"):
        batched.shock_decomposition_batched(T, R, x, e, Z=np.zeros((2, M + 1)))
    with pytest.raises(ValueError, match="Z must be"):
        batched.shock_decomposition_batched(T, R, x, e, Z=np.zeros((NB + 1, 2, M)))
    with pytest.raises(ValueError, match="status"):
        batched.shock_decomposition_batched(T, R, x, e, status=np.zeros(NB + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="at most 96"):
        batched.shock_decomposition_batched(*_inputs(m=97))


def test_variables_are_checked(no_library):
    with pytest.raises(ValueError, match="twice"):
        batched.shock_decomposition_batched(*_inputs(), variables=[1, 4, 1])
    with pytest.raises(ValueError, match="within 0"):
        batched.shock_decomposition_batched(*_inputs(), variables=[0, M])
    with pytest.raises(ValueError, match="nothing requested"):
        batched.shock_decomposition_batched(*_inputs(), variables=[])


def _raw(T, R, x, e, *, groups=None, g=None, var=None, n_out=None, Z=None, p=0, n_paths=1, T_len=None, remainder=1, contrib=True,
         obs=False):
    """The host twin called directly: the return code, with everything after the refusal never reached on a machine without a GPU."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nb, m, k = R.shape
    T_len = e.shape[-2] if T_len is None else T_len
    g = (k if groups is None else len(set(groups))) if g is None else g
    grp = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    vi = None if var is None else np.ascontiguousarray(var, dtype=np.int32)
    n_out = (m if var is None else len(var)) if n_out is None else n_out
    C = g + 1 + remainder
    c_out = np.empty((nb, n_paths, T_len, n_out, C)) if contrib else None
    o_out = np.empty((nb, n_paths, T_len, max(p, 1), C)) if obs else None
    return lib.dsge_shock_decomposition_batched_host(ptr(T), ptr(R), ptr(e), ptr(x), ptr(grp), g, ptr(vi), n_out, ptr(Z), 0, None, nb, m,
                                                     k, p, n_paths, T_len, remainder, ptr(c_out), ptr(o_out))


def test_the_library_refuses_sizes_before_any_device():
    big, bad = _lib.ERR_TOO_LARGE, _lib.ERR_INVALID
    assert _raw(*_inputs(m=20, k=16)) == big  # 16 groups: G = 17 columns
    assert b"15 groups" in _lib.load().dsge_last_error()
    assert _raw(*_inputs(m=97)) == big
    assert _raw(*_inputs(m=96, k=40)) == big  # [T | R] beyond the LDS
    assert _raw(*_inputs(), Z=np.zeros((17, M)), p=17, obs=True) == big
    with pytest.raises(_lib.DsgeTooLargeError, match="15 groups"):
        batched.shock_decomposition_batched(*_inputs(m=20, k=16))
    assert _raw(*_inputs(), T_len=0) == bad
    assert _raw(*_inputs(m=3, k=4)) == bad


def test_the_library_refuses_malformed_calls_before_any_device():
    bad = _lib.ERR_INVALID
    T, R, x, e = _inputs()
    assert _raw(T, R, x, e, groups=[0, 0, 2], g=3) == bad  # group 1 holds no shock: not a partition into 3
    assert b"every group" in _lib.load().dsge_last_error()
    assert _raw(T, R, x, e, groups=[0, 1, 3], g=3) == bad
    assert _raw(T, R, x, e, groups=[0, -1, 1], g=2) == bad
    assert _raw(T, R, x, e, g=2) == bad  # NULL list means one group per shock
    assert _raw(T, R, x, e, var=[1, 4, 1]) == bad
    assert b"twice" in _lib.load().dsge_last_error()
    assert _raw(T, R, x, e, var=[1, M]) == bad
    assert _raw(T, R, x, e, n_out=M - 1) == bad  # NULL list means all variables
    assert _raw(T, R, x, e, contrib=False) == bad  # nothing requested
    assert _raw(T, R, x, e, contrib=False, obs=True) == bad  # obs_out without Z
    assert _raw(None, R, x, e) == bad
    assert _raw(T, R, None, e) == bad
    assert _raw(T, R, x, None, T_len=T_LEN) == bad


def test_the_abi_names_the_entry():
    assert _lib.ABI_VERSION >= 14
    sig = [name for name, _ in _lib.SIGNATURES["dsge_shock_decomposition_batched"]]
    assert sig[-1] == "stream" and [name for name, _ in _lib.SIGNATURES["dsge_shock_decomposition_batched_host"]] == sig[:-1]
