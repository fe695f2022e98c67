"""Historical shock decomposition in numpy (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the definition of
``dsge_shock_decomposition_batched`` (include/dsge_hip.h) restated one component at a time -- a separate vector recursion per
group and for the initial condition, no packed tile -- and, independently, the convolution form with explicit matrix powers.

One draw and one path: T (m, m), R (m, k), x (T_len, m), e (T_len, k) with e[0] never read (NaN by the smoother's definition).
Component order: groups 0 .. g-1, initial condition, remainder."""
import numpy as np


def group_of_shock(groups, k):
    """``groups`` (None or a partition of 0 .. k-1 as a sequence of index sequences) -> the group of every shock, g."""
    if groups is None:
        return np.arange(k), k
    of = np.full(k, -1)
    for c, members in enumerate(groups):
        of[list(members)] = c
    assert (of >= 0).all()
    return of, len(groups)


def components(T, R, x, e, groups=None, remainder=True):
    """(T_len, m, C): one recursion per component."""
    T_len, m = x.shape
    of, g = group_of_shock(groups, R.shape[1])
    out = np.zeros((T_len, m, g + 1 + bool(remainder)))
    for c in range(g):
        Rc = R[:, of == c]
        v = np.zeros(m)
        for t in range(1, T_len):
            v = T @ v + Rc @ e[t, of == c]
            out[t, :, c] = v
    v = x[0].copy()
    out[0, :, g] = v
    for t in range(1, T_len):
        v = T @ v
        out[t, :, g] = v
    if remainder:
        s = np.zeros((T_len, m))
        for c in range(g + 1):  # ascending, as the definition says
            s = s + out[:, :, c]
        out[:, :, g + 1] = x - s
    return out


def decomposition(T, R, x, e, groups=None, variables=None, Z=None, remainder=True):
    """dict(contributions (T_len, n_out, C), observed (T_len, p, C) or None) of one draw and path."""
    comp = components(T, R, x, e, groups, remainder)
    rows = np.arange(x.shape[1]) if variables is None else np.asarray(variables, dtype=int)
    return dict(contributions=comp[:, rows, :], observed=None if Z is None else np.einsum("pi,tic->tpc", Z, comp))


def batch_decomposition(T, R, x, e, groups=None, variables=None, Z=None, remainder=True):
    """The same for T (nb, m, m), R (nb, m, k), x (nb, n_paths, T_len, m), e (nb, n_paths, T_len, k), Z (p, m) or (nb, p, m)."""
    nb, n_paths = x.shape[:2]
    one = [[decomposition(T[b], R[b], x[b, s], e[b, s], groups, variables, None if Z is None else (Z if Z.ndim == 2 else Z[b]),
                          remainder) for s in range(n_paths)] for b in range(nb)]
    stack = lambda key: np.array([[one[b][s][key] for s in range(n_paths)] for b in range(nb)])  # noqa: E731
    return dict(contributions=stack("contributions"), observed=None if Z is None else stack("observed"))


def convolution(T, R, x, e, groups=None):
    """(T_len, m, g + 1) from the closed form: component c at t is sum_{s=1..t} T^(t-s) R[:, J_c] e_s[J_c], the initial
    condition T^t x_0 -- explicit matrix powers, no recursion on the components."""
    T_len, m = x.shape
    of, g = group_of_shock(groups, R.shape[1])
    powers = [np.linalg.matrix_power(T, h) for h in range(T_len)]
    out = np.zeros((T_len, m, g + 1))
    for t in range(T_len):
        for c in range(g):
            J = of == c
            for s in range(1, t + 1):
                out[t, :, c] += powers[t - s] @ (R[:, J] @ e[s, J])
        out[t, :, g] = powers[t] @ x[0]
    return out


def exact_path(T, R, e, x0):
    """x with x[0] = x0 and x[t] = T x[t-1] + R e[t]: a path whose remainder is rounding."""
    x = np.empty((e.shape[0], T.shape[0]))
    x[0] = x0
    for t in range(1, e.shape[0]):
        x[t] = T @ x[t - 1] + R @ e[t]
    return x
