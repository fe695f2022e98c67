"""GPU box: record what the cycle-reduction kernels return, bit for bit, into tests/golden/cr_bitwise_parent.npz.

    python tools/make_cr_bitwise_golden.py [out.npz]

Run it on a build of the commit whose results are to be pinned (the PARENT of a change that must not move a rounding);
tests/test_gpu_cr_bitwise.py then compares every array of a later build with np.array_equal.  The existing bit-identity
tests compare kernels that share the blocked elimination with each other and cannot see a change that moves all of them
together; this fixture can.

The inputs are regenerated from seeds (workloads.sw_shaped_system / sw_shaped_batch) and pinned by a SHA-256 of their
bytes (`<case>/input_sha256`), so that a failing comparison can be told from a generator that drifted.  Cases, four draws
each unless noted -- the smallest shapes at which each path of gauss_jordan_blocked / crc_iterate can go wrong:

    n17, n24            3 x 3 tile, partial and full last panel
    n29, n30, n32       4 x 4 tile (two wavefronts per SIMD), last panel of width 1, 2, 4
    n40                 5 x 5 tile, no static variables
    sw_fused            SW-shaped draws 0..3 through the fused deflated launch (40 -> 30): T, R, logp
    sw752_fused         SW-shaped draw 752 (refines in every iteration), fused launch
    sw752_compact       the same draw through cr_compact_kernel
    n56_wide            one 56-variable system on cr_wide_kernel
    sw_grad             the gradient entry on SW-shaped draws 0..3 (adjoint eliminations): logp and every cotangent
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "cr_bitwise_parent.npz")
TOL, MAX_ITER = 1e-8, 1000
SEED0 = 7100  # sw_shaped_system(SEED0 + 10 * n + draw, ...) for the plain cycle-reduction cases
# name -> (n, n_state, n_lead, draws): n_state + n_lead = n (no static variables, nothing to deflate)
PLAIN = {
    "n17": (17, 9, 8, 4),
    "n24": (24, 14, 10, 4),
    "n29": (29, 16, 13, 4),
    "n30": (30, 18, 12, 4),
    "n32": (32, 18, 14, 4),
    "n40": (40, 24, 16, 4),
    "n56_wide": (56, 30, 26, 1),
}
CASES = tuple(PLAIN) + ("sw_fused", "sw752_fused", "sw752_compact", "sw_grad")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _plain_inputs(name):
    from geconpy_amd import workloads as wl

    n, ns, nl, draws = PLAIN[name]
    sysm = [wl.sw_shaped_system(SEED0 + 10 * n + i, n=n, n_state=ns, n_lead=nl, k=7) for i in range(draws)]
    return tuple(np.stack([s[j] for s in sysm]) for j in range(3))


def run_case(name):
    """One case on the GPU: dict of arrays (inputs' checksum + everything the entry point returned)."""
    from geconpy_amd import batched
    from geconpy_amd import workloads as wl

    if name in PLAIN:
        A, B, C = _plain_inputs(name)
        T, st, it = batched.cycle_reduction_batched(A, B, C, max_iter=MAX_ITER, tol=TOL)
        return dict(input_sha256=_sha(A, B, C), T=T, status=st, n_iter=it)
    first, count = (752, 1) if name.startswith("sw752") else (0, 4)
    b = wl.sw_shaped_batch(count, first_draw=first)
    sha = _sha(b["A"], b["B"], b["C"], b["D"], b["sigma"])
    if name == "sw752_compact":
        T, st, it = batched.cycle_reduction_batched(b["A"], b["B"], b["C"], max_iter=MAX_ITER, tol=TOL)
        return dict(input_sha256=sha, T=T, status=st, n_iter=it)
    om = wl.sw_shaped_observation_model()
    if name == "sw_grad":
        g = batched.solve_kalman_logp_grad_batched(b["A"], b["B"], b["C"], b["D"], b["sigma"] ** 2, om["Z"], om["y"],
                                                   Hdiag=om["Hdiag"], tol=TOL, max_iter=MAX_ITER)
        out = {k: np.asarray(v) for k, v in g.items() if isinstance(v, np.ndarray)}
        assert {"logp", "status", "A_bar", "B_bar", "C_bar", "D_bar", "q_bar"} <= set(out), sorted(out)
        return dict(input_sha256=sha, **out)
    r = batched.solve_kalman_logp_batched(b["A"], b["B"], b["C"], b["D"], b["sigma"] ** 2, om["Z"], om["y"], Hdiag=om["Hdiag"],
                                          q_mode=1, tol=TOL, max_iter=MAX_ITER, return_policy=True)
    return dict(input_sha256=sha, T=r["T"], R=r["R"], status=r["status"], n_iter=r["n_iter"], logp=r["logp"])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    flat = {}
    for name in CASES:
        res = run_case(name)
        print(name, {k: (v.shape, str(v.dtype)) for k, v in res.items()}, "status", res["status"].tolist(),
              "n_iter", res["n_iter"].tolist() if "n_iter" in res else None, flush=True)
        for k, v in res.items():
            flat[f"{name}/{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **flat)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
