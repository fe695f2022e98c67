"""GPU box: record what the fused likelihood call returns -- logp and status, the caller asks for neither T nor R -- on the
cases of tests/test_gpu_cr_static_skip.py, bit for bit, into tests/golden/cr_static_skip_parent.npz.

    python tools/make_cr_static_skip_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned: the PARENT of the change that lets the one-launch deflated
cycle reduction leave the static rows of T and R at zero where the filter behind it reads none of them (dsge_cr_fused.hpp,
phase 3; docs/design/cycle_reduction.md 4.1i).  The test then compares a later build with np.array_equal.  Batches of 4 to 8
draws, T_len <= 16, every call with n_static_hint set; the systems are wl.sw_shaped_system with small shapes (states first,
then the static variables, then the forward-looking ones).  The inputs are regenerated from seeds and pinned by a SHA-256.

    base_n8, base_n12       the smallest systems launch_cr_deflated's rule deflates (h = 2 of 8, h = 3 of 12).  No one-launch
                            instance exists below 17 variables (launch_cr_fused): they run cr_deflate -> cr_compact ->
                            cr_inflate, which always forms the static rows
    base_n20                n = 20, h = 4: the smallest one-launch instance (3, 2)
    base_n37                n = 37 below the 40-row tile: the clamped loads (of A, C and of Z)
    base_n40                the benchmark's shape, h = 10
    base_n48                n = 48, h = 8: three columns per lane (the (6, 5, 3) instance)
                            -- in all of them Z selects states only
    obs_static_n12/_n40     one of the p observations is on a static variable: every row is needed
    mixed_n40               ONE Z that observes variable 18; draws 1, 4, 6 have 19 states (18 is a state there, 9 static variables
                            19..27), the others 18 states (18 is the first of 10 static variables); hint 9
    zbatched_n40            z_batched = 1: odd draws observe the static variable 18 + draw, even draws states only
    p8_n40, p1_n40          eight observations / one
    p9_n40                  nine: beyond the filter's fast kernels and beyond what the solver is told (p <= 8)
    more_static_n40         hint 8 of 10 static variables (18..25 deflated, 26 and 27 stay in the reduced system); draw 0 observes
                            26 (not deflated), draw 1 observes 20 (deflated), the others states only (z_batched = 1)
    rst_singular_n40        draw 2: the column of B of the static variable 21 is exactly zero (R_st singular: hand-over)
    nonconv_n40             max_iter = 2: no draw converges
    handed_on_n12/_n20      a dense Z (no selector) with zero columns on the static variables, z_selector_hint = 0: the general
                            filter, which reads T, R, sym(R Q R') and P0 of all n variables
"""
from __future__ import annotations

import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "cr_static_skip_parent.npz")
TOL, MAX_ITER = 1e-8, 1000
SEED0 = 160000
# name -> (n, n_state, n_lead, k, hint, draws, p, T_len)
SHAPES = {
    "base_n8": (8, 3, 3, 2, 2, 4, 2, 12),
    "base_n12": (12, 5, 4, 3, 3, 4, 3, 12),
    "base_n20": (20, 9, 7, 3, 4, 4, 3, 12),
    "base_n37": (37, 17, 11, 7, 9, 4, 5, 12),
    "base_n40": (40, 18, 12, 7, 10, 6, 7, 16),
    "base_n48": (48, 22, 18, 7, 8, 4, 7, 12),
    "obs_static_n12": (12, 5, 4, 3, 3, 4, 3, 12),
    "obs_static_n40": (40, 18, 12, 7, 10, 4, 7, 12),
    "mixed_n40": (40, 18, 12, 7, 9, 8, 7, 12),
    "zbatched_n40": (40, 18, 12, 7, 10, 6, 7, 12),
    "p8_n40": (40, 18, 12, 7, 10, 4, 8, 12),
    "p1_n40": (40, 18, 12, 7, 10, 4, 1, 12),
    "p9_n40": (40, 18, 12, 7, 10, 4, 9, 12),
    "more_static_n40": (40, 18, 12, 7, 8, 4, 7, 12),
    "rst_singular_n40": (40, 18, 12, 7, 10, 4, 7, 12),
    "nonconv_n40": (40, 18, 12, 7, 10, 4, 7, 12),
    "handed_on_n12": (12, 5, 4, 3, 3, 4, 3, 12),
    "handed_on_n20": (20, 9, 7, 3, 4, 4, 3, 12),
}
CASES = tuple(SHAPES)
MIXED_STATE_DRAWS = (1, 4, 6)
KEYS = ("logp", "status")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _selector(n, cols):
    Z = np.zeros((len(cols), n))
    Z[np.arange(len(cols)), cols] = 1.0
    return Z


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(A, B, C, D, sig, Z, y, Hdiag: read-only arrays; hint, max_iter, z_selector_hint) of a case."""
    from geconpy_amd import workloads as wl

    n, ns, nl, k, hint, nb, p, T_len = SHAPES[name]
    seed0 = SEED0 + 100 * CASES.index(name)
    b = wl.sw_shaped_batch(nb, seed0=seed0, n=n, n_state=ns, n_lead=nl, k=k)
    A, B, C, D, sig = (b[x].copy() for x in ("A", "B", "C", "D", "sigma"))
    rng = np.random.default_rng(seed0 + 99)
    Z = _selector(n, np.arange(p))  # states only (p <= n_state everywhere)
    max_iter, zsel = MAX_ITER, None
    if name.startswith("obs_static"):
        Z = _selector(n, list(range(p - 1)) + [ns + 1])
    elif name == "mixed_n40":
        for i in MIXED_STATE_DRAWS:
            A[i], B[i], C[i], D[i], _ = wl.sw_shaped_system(seed0 + 50 + i, n=n, n_state=ns + 1, n_lead=nl, k=k)
        Z = _selector(n, list(range(p - 1)) + [ns])
    elif name == "zbatched_n40":
        Z = np.stack([_selector(n, list(range(p - 1)) + [ns + i if i % 2 else p - 1]) for i in range(nb)])
    elif name == "more_static_n40":
        last = [ns + 8, ns + 2] + [p - 1] * (nb - 2)
        Z = np.stack([_selector(n, list(range(p - 1)) + [last[i]]) for i in range(nb)])
    elif name == "rst_singular_n40":
        B[2, :, ns + 3] = 0.0
    elif name == "nonconv_n40":
        max_iter = 2
    elif name.startswith("handed_on"):
        Z = np.zeros((p, n))
        dyn = np.r_[0:ns, n - nl:n]
        Z[:, dyn] = rng.standard_normal((p, len(dyn)))
        zsel = 0
    y = rng.normal(0, 0.02, (T_len, p))
    Hdiag = np.full(p, 1e-4)
    out = dict(A=A, B=B, C=C, D=D, sig=sig, Z=Z, y=y, Hdiag=Hdiag)
    for x in out.values():
        x.setflags(write=False)
    out.update(hint=hint, max_iter=max_iter, z_selector_hint=zsel)
    return out


def input_sha(name):
    a = inputs(name)
    return _sha(*(a[x] for x in ("A", "B", "C", "D", "sig", "Z", "y", "Hdiag")))


def static_mask(name):
    """(draw, variable): the columns of A and C are both exactly zero."""
    a = inputs(name)
    return ~((a["A"] != 0).any(axis=1) | (a["C"] != 0).any(axis=1))


def observed_mask(name):
    """(draw, variable): the column of the draw's Z has a non-zero entry."""
    a = inputs(name)
    nb, n = a["A"].shape[:2]
    return np.broadcast_to((a["Z"] != 0).any(axis=-2), (nb, n))


def one_launch_instance(n, k, h):
    """launch_cr_deflated's rule and the instances of launch_cr_fused (launch_solvers.hip): does the one-launch kernel take (n, h)?"""
    bs = lambda m: max(1, (m + 7) // 8)  # noqa: E731
    nd = n - h
    if h < 1 or nd < 4 or (bs(nd) == bs(n) and 5 * h < n) or k > 8 * bs(nd):
        return False
    ncol = h + 3 * nd + k
    if ncol > 192 or nd + k > 64:
        return False
    f, d = bs(n), bs(nd)
    two = {(3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (6, 4), (6, 5)}
    three = {(6, 5), (7, 5), (7, 6), (8, 6)}
    return (f, d) in (two if ncol <= 128 else three)


def expected_skip(name):
    """Per draw: the solver is told the observation model (p <= 8), the one-launch kernel takes the draw, and none of the `hint`
    static variables it deflates -- the first `hint` of the draw's static variables -- is observed."""
    n, _, _, k, hint, nb, p, _ = SHAPES[name]
    st, ob = static_mask(name), observed_mask(name)
    out = np.zeros(nb, dtype=bool)
    if p > 8 or not one_launch_instance(n, k, hint):
        return out
    for i in range(nb):
        idx = np.flatnonzero(st[i])
        out[i] = len(idx) >= hint and not ob[i, idx[:hint]].any()
    return out


def evaluate(name, out=None):
    """The fused likelihood call on the GPU (host twin).  out = dict(T=, R=): buffers the call fills as well."""
    from geconpy_amd import _frontend as F
    from geconpy_amd import batched

    a = inputs(name)

    def hints(v):
        return dict(n_state_hint=batched.state_hint(v["A"]),
                    z_selector_hint=batched.selector_hint(v["Z"]) if a["z_selector_hint"] is None else a["z_selector_hint"],
                    n_lead_hint=0)

    r = F.solve_kalman_logp(batched.HOST, a["A"], a["B"], a["C"], a["D"], a["sig"] ** 2, a["Z"], a["y"], d=None, Hdiag=a["Hdiag"],
                            q_mode=1, solver="cycle_reduction", tol=TOL, max_iter=a["max_iter"], jitter=batched.JITTER_DEFAULT,
                            missing_fill=batched.MISSING_FILL, hints=hints, options={"n_static_hint": a["hint"]}, out=out)
    return {key: np.asarray(v) for key, v in r.items() if v is not None}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        flat[f"{name}/input_sha256"] = input_sha(name)
        got = evaluate(name)
        for key in KEYS:
            flat[f"{name}/{key}"] = got[key]
        print(name, "status", got["status"].tolist(), "logp", got["logp"].tolist(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
