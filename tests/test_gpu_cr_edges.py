"""Edges of the cycle-reduction kernels that the recorded fixture of tests/test_gpu_cr_bitwise.py does not reach.

The column-compact kernel is bit-identical to the dense kernel by construction (it only drops additions of +0.0), and the
fused deflated launch to the three launches; so the dense kernel (cr_compact = 0, cr_deflation = 0) and the three launches
(cr_fused_deflation = 0) are the references here, and every array -- T, R, status, iteration counts -- is compared with
np.array_equal, and bit pattern against bit pattern on top of it (np.array_equal alone takes -0.0 for +0.0; compact against
dense on the state columns of T, see _compact_against_dense).  No tolerance, no draw left out.  The cases are the places where the position tables of the scatter (a pad column of the LDS tile stands in for
"no such column"), the register-resident right-hand sides of the final solve and the row order it leaves behind can go wrong:

    full2, full3     s + l equals the tile width exactly (2 x 2 blocks: n = 16, s = l = 8; 3 x 3: n = 24, s = l = 12): no
                     spare column in the products
    partial          n = 13: the last panel is partial; two variables are neither state nor lead
    overlap          n = 12, 8 states, 6 leads: variables 6 and 7 are both
    negzero          a -0.0 planted in an entry of B whose column is outside S and L, and in an entry of A
    (every batch)    one diverging draw, A and C scaled until the iterates hold Inf: status and output of the dense kernel
    fused_*          the fused launch on a small reduced system, k = 1 and k = 7 shock columns (a partial column block of the
                     final solve's right-hand sides): h = 4 static variables in n = 12 (no fused instance is built for that
                     tile pair: the launcher's own fall-back) and in n = 20 (tiles 3 / 2: the fused kernel itself)
    refine           SW-shaped draw 752, which refines in every iteration (tools/make_cr_bitwise_golden.py), compact against
                     dense and fused against three launches

test_inputs_converge_on_the_oracle needs no GPU: every draw that is not the planted diverging one converges on the CPU
oracle, so that no comparison here is one of two failures.
"""
import functools

import numpy as np
import pytest

import oracle
from geconpy_amd import workloads as wl

TOL, MAX_ITER = 1e-8, 1000
NB = 8
BAD = 5  # the diverging draw of every batch

# name -> (n, n_state, n_lead, k)
PLAIN = {
    "full2": (16, 8, 8, 3),
    "full3": (24, 12, 12, 3),
    "partial": (13, 6, 5, 3),
    "overlap": (12, 8, 6, 3),
    "negzero": (13, 6, 5, 3),
}
FUSED = {
    "fused_n12_k1": (12, 5, 3, 1),
    "fused_n12_k7": (12, 5, 3, 7),
    "fused_n20_k1": (20, 9, 7, 1),
    "fused_n20_k7": (20, 9, 7, 7),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """A, B, C, D, sigma of a case (read-only arrays): NB draws, draw BAD scaled to overflow."""
    n, ns, nl, k = {**PLAIN, **FUSED}[name]
    b = wl.sw_shaped_batch(NB, n=n, n_state=ns, n_lead=nl, k=k)
    A, B, C, D, sig = (b[x].copy() for x in ("A", "B", "C", "D", "sigma"))
    if name == "negzero":
        assert not (A[:, :, 6:8] != 0).any() and not (C[:, :, 6:8] != 0).any()  # columns 6, 7: neither state nor lead
        B[:, 2, 6] = -0.0
        A[:, 4, 1] = -0.0
    A[BAD] *= 1e160  # X = A1^-1 [A0 | A2] ~ 1e160, the products A0 X overflow in the first iteration
    C[BAD] *= 1e160
    for x in (A, B, C, D, sig):
        x.setflags(write=False)
    return A, B, C, D, sig


def _same(got, want, what, bits_where=None):
    """np.array_equal, and equal bit patterns on top of it (all entries, or the columns `bits_where` of the last axis)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), what
    if bits_where is not None:
        got, want = np.ascontiguousarray(got[..., bits_where]), np.ascontiguousarray(want[..., bits_where])
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{what}: bit patterns (signed zeros) differ"


@pytest.mark.parametrize("name", sorted({**PLAIN, **FUSED}))
def test_inputs_converge_on_the_oracle(name):
    A, B, C, D, _ = _inputs(name)
    for i in range(NB):
        T, converged, _ = oracle.cycle_reduction_core(A[i], B[i], C[i], MAX_ITER, TOL)
        assert bool(converged) == (i != BAD), (name, i)
    with np.errstate(all="ignore"):  # the diverging draw: Inf in the first iterate already
        X = np.linalg.solve(B[BAD], A[BAD])
        assert np.isinf(A[BAD] @ X).any()


def _refine_inputs():
    b = wl.sw_shaped_batch(1, first_draw=752)
    return tuple(b[x] for x in ("A", "B", "C", "D", "sigma"))


def _compact_against_dense(A, B, C, bad=None):
    from geconpy_amd import batched

    got = batched.cycle_reduction_batched(A, B, C, max_iter=MAX_ITER, tol=TOL)
    want = batched.cycle_reduction_batched(A, B, C, max_iter=MAX_ITER, tol=TOL, options={"cr_compact": 0, "cr_deflation": 0})
    # The columns of T outside S are computed by neither kernel's arithmetic in the same way: the dense kernel negates an exact
    # +0.0 there (-0.0), the compact kernel writes +0.0 -- on every commit, nothing the position tables touch.  Bit patterns are
    # therefore compared on the state columns, where every entry comes out of the elimination.
    states = (A != 0).any(axis=(0, 1))
    _same(got[0], want[0], "T", bits_where=states)
    for g, w, what in zip(got[1:], want[1:], ("status", "n_iter")):
        _same(g, w, what)
    st = want[1]
    ok = np.ones(len(st), dtype=bool)
    if bad is not None:
        ok[bad] = False
        assert st[bad] != 0 and not want[0][bad].any()
    assert (st[ok] == 0).all(), st
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_compact_equals_dense(name):
    A, B, C, _, _ = _inputs(name)
    T, _, _ = _compact_against_dense(A, B, C, bad=BAD)
    if name == "negzero":  # the planted zeros did not turn the columns into states or leads: T is zero there, in both kernels
        assert not T[:, :, 6:8].any()


def _policy(A, B, C, D, sig, options):
    from geconpy_amd import batched

    n, k = D.shape[1:]
    p = min(3, k)
    Z = np.zeros((p, n))
    Z[np.arange(p), np.arange(p)] = 1.0
    y = np.random.default_rng(n + k).normal(0, 0.02, (8, p))
    r = batched.solve_kalman_logp_batched(A, B, C, D, sig ** 2, Z, y, Hdiag=np.full(p, 1e-4), q_mode=1, tol=TOL, max_iter=MAX_ITER,
                                          return_policy=True, options=options)
    return {key: r[key] for key in ("T", "R", "status", "n_iter", "logp")}


def _fused_against_three_launches(A, B, C, D, sig, bad=None):
    from geconpy_amd import batched

    h = batched.static_hint(A, C)
    got = _policy(A, B, C, D, sig, {"cr_fused_deflation": 1, "n_static_hint": h})
    want = _policy(A, B, C, D, sig, {"cr_fused_deflation": 0, "n_static_hint": h})
    for key in ("T", "R", "status", "n_iter", "logp"):
        _same(got[key], want[key], key)
    st = want["status"]
    ok = np.ones(len(st), dtype=bool)
    if bad is not None:
        ok[bad] = False
        assert st[bad] != 0 and not want["T"][bad].any() and not want["R"][bad].any()
    assert (st[ok] == 0).all(), st
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_equals_three_launches_on_a_small_reduced_system(name):
    A, B, C, D, sig = _inputs(name)
    assert _fused_against_three_launches(A, B, C, D, sig, bad=BAD) == 4


@pytest.mark.gpu
def test_refining_draw():
    A, B, C, D, sig = _refine_inputs()
    _compact_against_dense(A, B, C)
    assert _fused_against_three_launches(A, B, C, D, sig) == 10
