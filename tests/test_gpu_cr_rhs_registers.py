"""The compact cycle reduction eliminates its right-hand sides in registers; the dense kernel keeps them in LDS.

crc_iterate (csrc/dsge_cr_compact.hpp) hands the register block of R = [A0c | A2c] to gauss_jordan_blocked_rhs: per panel the
eight lanes that own a pivot row publish that row of their block, selected by its position inside the block.  The random
systems of tests/golden/cr_bitwise_parent.npz pivot close to the diagonal and do not choose which lanes own a panel's pivot
rows, nor at which position; the systems here do.  They are built as workloads.sw_shaped_system builds its own, with
M = P + 0.05 noise for a permutation matrix P (partial pivoting then follows P, but for a rare pivot), rho(T*[S,S]) = 0.6 and
rho(G) = 0.3 (six iterations at tol = 1e-9), and three permutations per size, BS = ceil(n / 8) being the panel width:

    block_row       each panel's columns go to the rows of one block row, reversed: one set of owner lanes per panel, every
                    position inside the block
    position_first  rows ordered by their position inside the block first: a panel's pivots sit in BS different block rows
    reversal        column c pivots on row n - 1 - c

The reference is the dense kernel (cr_compact = 0 sends the same entry to cr_kernel), whose elimination is the untouched LDS
form: T, status and iteration counts are compared with np.array_equal, status 0 is required everywhere.  What the generator
is there for is asserted from a numpy replay of the first elimination, so that a change of the generator cannot empty the test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
# (n, n_state, n_lead): the 2-, 3-, 4- and 5-wide tiles, last panels of one and two columns, s + l equal to the tile and far below it
SIZES = [(13, 5, 4), (17, 9, 8), (29, 12, 3), (30, 18, 12), (32, 20, 12), (40, 24, 16), (40, 8, 4)]
FAMILIES = ("block_row", "position_first", "reversal")
SEEDS = (0, 1, 2, 3)
REFINE_SIZE = (30, 18, 12)
REFINE_SCALE = 1e-5
REFINE_RATIO = 3e3  # cr_refine_ratio<4>(): the tiles of 25 .. 40 variables refine beyond it


def _bs(n):
    return (n + 7) // 8


def pivot_rows(n, family):
    """rows[c]: the row of P that holds the one of column c, i.e. the pivot row of column c."""
    bs = _bs(n)
    if family == "block_row":
        rows = []
        for j0 in range(0, n, bs):
            bw = min(bs, n - j0)
            rows += [j0 + bw - 1 - a for a in range(bw)]
        return np.array(rows)
    if family == "position_first":
        return np.array(sorted(range(n), key=lambda r: (r % bs, r // bs)))
    if family == "reversal":
        return np.arange(n)[::-1].copy()
    raise ValueError(family)


def _rescale(M, target):
    return M * (target / np.max(np.abs(np.linalg.eigvals(M))))


def system(seed, n, ns, nl, family):
    rng = np.random.default_rng([9100 + seed, n, ns, nl, FAMILIES.index(family)])
    T_star = np.zeros((n, n))
    T_star[:ns, :ns] = _rescale(rng.standard_normal((ns, ns)), 0.6)
    T_star[ns:, :ns] = 0.3 * rng.standard_normal((n - ns, ns))
    G = np.zeros((n, n))
    G[:, n - nl:] = rng.standard_normal((n, nl))
    G = _rescale(G, 0.3)
    P = np.zeros((n, n))
    P[pivot_rows(n, family), np.arange(n)] = 1.0
    M = P + 0.05 * rng.standard_normal((n, n))
    C = M @ G
    B = M - C @ T_star
    A = -M @ T_star
    return A, B, C, T_star


def batch(size, refine=False):
    """The 12 systems of a size (family-major, then seed) and their families; refine: one equation scaled by REFINE_SCALE."""
    n, ns, nl = size
    A, B, C, fam = [], [], [], []
    for f in FAMILIES:
        for seed in SEEDS:
            a, b, c, _ = system(seed, n, ns, nl, f)
            if refine:
                row = pivot_rows(n, f)[n - 1]  # the equation that pivots the last column: it waits for its turn, the other pivots stay O(1)
                a[row] *= REFINE_SCALE
                b[row] *= REFINE_SCALE
                c[row] *= REFINE_SCALE
            A.append(a)
            B.append(b)
            C.append(c)
            fam.append(f)
    return np.stack(A), np.stack(B), np.stack(C), fam


def replay_first_elimination(B):
    """Gauss-Jordan with partial pivoting among the rows not yet used, as the blocked elimination chooses its pivots (the panel's
    columns carry every earlier update when they are searched).  Returns the pivot row of every column and the pivots."""
    W = np.array(B, dtype=np.float64)
    n = W.shape[0]
    free = np.ones(n, dtype=bool)
    rows, piv = [], []
    for c in range(n):
        r = int(np.argmax(np.where(free, np.abs(W[:, c]), -1.0)))
        free[r] = False
        rows.append(r)
        piv.append(W[r, c])
        f = W[:, c] / W[r, c]
        f[r] = 0.0
        W -= np.outer(f, W[r])
    return np.array(rows), np.array(piv)


def _panels(n):
    bs = _bs(n)
    return [range(j0, min(n, j0 + bs)) for j0 in range(0, n, bs)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "n%d_s%d_l%d" % s)
def test_generator_chooses_owner_lanes_and_positions(size):
    n = size[0]
    bs = _bs(n)
    _, B, _, fam = batch(size)
    positions = set()
    for b, f in zip(B, fam):
        rows, _ = replay_first_elimination(b)
        positions |= {int(r) % bs for r in rows}
        full = [cols for cols in _panels(n) if len(cols) == bs]
        one_block_row = sum(len({int(rows[c]) // bs for c in cols}) == 1 and {int(rows[c]) % bs for c in cols} == set(range(bs))
                            for cols in full)
        all_distinct = sum(len({int(rows[c]) // bs for c in cols}) == bs for cols in full)
        # (the noise may move a pivot or two away from P: most of the full panels, not every one)
        if f == "block_row":
            assert 2 * one_block_row > len(full), (f, rows)
        if f == "position_first":
            assert 2 * all_distinct > len(full), (f, rows)
        if f == "reversal":
            assert np.count_nonzero(rows == pivot_rows(n, f)) > n // 2, (f, rows)
    assert positions == set(range(bs))


def _solve_both(A, B, C, **extra):
    from geconpy_amd import batched

    dense = batched.cycle_reduction_batched(A, B, C, tol=TOL, options={"cr_compact": 0})
    compact = batched.cycle_reduction_batched(A, B, C, tol=TOL, options=dict(extra) or None)
    return dense, compact


def _assert_same(dense, compact):
    for name, d, c in zip(("T", "status", "n_iter"), dense, compact):
        assert np.array_equal(d, c), (name, np.argwhere(np.asarray(d) != np.asarray(c))[:8].tolist())
    assert not dense[1].any(), dense[1].tolist()
    assert not compact[1].any(), compact[1].tolist()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "n%d_s%d_l%d" % s)
def test_compact_equals_dense(size):
    A, B, C, _ = batch(size)
    dense, compact = _solve_both(A, B, C)
    _assert_same(dense, compact)
    if _bs(size[0]) == 4:  # the 4 x 4 tile has a second instance (one wavefront per SIMD)
        from geconpy_amd import batched

        _assert_same(dense, batched.cycle_reduction_batched(A, B, C, tol=TOL, options={"cr_two_waves": 0}))


def test_refining_systems_compact_equals_dense():
    """One equation scaled by 1e-5: the solvent is the same, the pivots of the first elimination span far more than the
    refinement rule allows, so both kernels take the refinement branch -- on other draws than the SW-shaped draw 752."""
    A, B, C, _ = batch(REFINE_SIZE, refine=True)
    for b in B:
        _, piv = replay_first_elimination(b)
        ratio = np.max(np.abs(piv)) / np.min(np.abs(piv))
        assert ratio > 10 * REFINE_RATIO, ratio
    _assert_same(*_solve_both(A, B, C))


def test_scan_compact_equals_dense():
    from geconpy_amd import _lib, batched

    A, B, C, _ = batch(REFINE_SIZE)
    with _lib.options_scope({"cr_compact": 0}):
        dense = batched.scan_cycle_reduction_batched(A, B, C)
    _assert_same(dense, batched.scan_cycle_reduction_batched(A, B, C))
