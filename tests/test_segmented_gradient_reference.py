"""CPU: keeps the autograd reference of the gradient across dated structural breaks (tests/segmented_gradient_reference.py) honest
without a device, on EVERY device accuracy case of tests/segmented_filter_cases.py:

- its value equals ``segmented_filter_reference`` (the numpy chain of ``oracle.kalman_filter_logp``) to 1e-12 relative;
- its gradient equals a second formulation -- the stationary P0 by ``lyapunov_doubling`` instead of the Kronecker solve -- to 1e-10 of
  each block's largest entry, every draw, every entry.  Measured: at most 7.8e-14 (``size_dense64_p16``);
- along 8 random UNIT directions per block (draw 0; ||u||_2 = 1) its directional derivative equals central differences of the value on
  a Romberg ladder, the difference taken per period, to FD_BAR = 1e-10 of the block's largest entry.  The (case, block) pairs
  that float64 differences cannot resolve are listed in FD_ROUNDING with the measured figure and the cause, and are held to 1e-8;
  every other block of every case meets 1e-10 (the largest not listed: 3.6e-11, q_bar of ``s8``).  A variance that is exactly zero
  is at the boundary of its domain and is not stepped across (its entry is held by the second formulation);
- from the reference alone: finite logp, cond_2(F_t) <= 1e4, and no cotangent block identically zero unless the case says so
  (``zero_blocks``), so that the device test cannot pass on zeros.

And ``launch_kalman_seg_grad.hip`` is compiled for gfx950: no kernel in it may use scratch memory."""
import os
import re

import numpy as np
import pytest

from tests import segmented_filter_cases as K
from tests import segmented_gradient_reference as G
from tests.segmented_filter_reference import innovation_conditions

VALUE_RTOL, SECOND_BAR, FD_BAR, FD_ROUNDING_BAR, N_DIRECTIONS = 1e-12, 1e-10, 1e-10, 1e-8, 8
# (case, block) -> (cause, measured): what float64 central differences do not resolve to 1e-10 of the block's scale, held to
# FD_ROUNDING_BAR.  One cause throughout: the rounding noise of the differenced terms, eps |ll_t| cond(F_t) / h, against a derivative
# along a unit direction that is small next to the block's largest entry.  These are the panels in which a period right behind a
# break or a missing entry has its largest innovation condition (``h`` and ``q`` enter F_t at the scale H = 1e-5, where the usable
# steps are shortest), and the full covariance per draw, whose block is dominated by one entry.  The autograd second formulation
# holds the same blocks to 1e-10.
_NOISE = "rounding noise of the differenced terms exceeds 1e-10 of the block's scale at every step of the ladder"
FD_ROUNDING = {
    ("s8", "h_bar"): (_NOISE, 2.3e-10),
    ("break_first", "q_bar"): (_NOISE, 4.5e-10),
    ("break_first", "h_bar"): (_NOISE, 5.0e-10),
    ("miss_entry_at_boundary", "h_bar"): (_NOISE, 1.0e-9),
    ("fill_marker_at_boundary", "q_bar"): (_NOISE, 1.1e-10),
    ("fill_marker_at_boundary", "h_bar"): (_NOISE, 4.6e-9),
    ("q_full_batched", "Q_bar"): (_NOISE, 3.8e-9),
}
BLOCKS = ("T_bar", "R_bar", "q_bar", "Z_bar", "d_bar", "h_bar", "shift_bar", "a0_bar", "P0_bar")


def _blocks(c):
    return tuple("Q_bar" if key == "q_bar" and c["q_mode"] in ("full", "full_batched") else key for key in BLOCKS)


def zero_blocks(c):
    """The blocks the case says must be identically zero: P0_bar without a given P0 (the stationary covariance is a function of
    T_0, R_0, Q_0), shift_bar with one segment (there is no boundary)."""
    return ({"P0_bar"} if c["P0"] is None else set()) | ({"shift_bar"} if len(c["seg_start"]) == 1 else set())


@pytest.mark.parametrize("name", G.GRADIENT_CASES)
def test_value_conditions_and_no_block_is_zero_by_accident(name):
    c, ref = G.case(name), G.case_reference(name)
    numpy_ref = K.reference_of(c)
    worst = 0.0
    for b, res in numpy_ref.items():  # (``segmented_filter_cases.check_conditions``, for a case of either list)
        assert np.isfinite(res["logp"]) and np.isfinite(res["ll"]).all(), (name, b)
        worst = max(worst, innovation_conditions(c["y"], K.draw(c, b), c["seg_start"], res).max())
    assert worst <= K.COND_MAX, (name, worst)
    for b, r in ref.items():
        want = numpy_ref[b]["logp"]
        err = abs(r["logp"] - want) / abs(want)
        print(f"{name} draw {b}: logp {err:.2e} cond {worst:.3g}")
        assert np.isfinite(r["logp"]) and err <= VALUE_RTOL
        for key in _blocks(c):
            assert np.isfinite(r[key]).all(), (name, b, key)
            if key in zero_blocks(c):
                assert not r[key].any(), (name, b, key)
            else:
                assert np.abs(r[key]).max() > 0.0, (name, b, key, "identically zero")
        assert not r["shift_bar"][0].any()  # row 0 is never read
        if c["P0"] is not None:
            assert np.abs(r["P0_bar"]).max() > 0.0
        if name == "zero_shock_one_segment":  # a shock without variance still has a gradient: the block is not zero there either
            assert r["q_bar"][1, 1] != 0.0


@pytest.mark.parametrize("name", G.GRADIENT_CASES)
def test_gradient_equals_the_second_formulation(name):
    c, ref = G.case(name), G.case_reference(name)
    other = G.reference(c, lyapunov="doubling")
    worst = 0.0
    for b, r in ref.items():
        assert abs(other[b]["logp"] - r["logp"]) <= VALUE_RTOL * abs(r["logp"])
        for key in _blocks(c):
            scale = np.abs(r[key]).max()
            if scale == 0.0:
                assert not other[b][key].any()
                continue
            worst = max(worst, np.abs(other[b][key] - r[key]).max() / scale)
    print(f"{name}: kronecker against doubling {worst:.2e}")
    assert worst <= SECOND_BAR


@pytest.mark.parametrize("name", G.GRADIENT_CASES)
def test_gradient_equals_central_differences_along_random_directions(name):
    c, r = G.case(name), G.case_reference(name)[0]
    leaves, full = G.draw_leaves(c, 0, grad=False)
    rng = np.random.default_rng([11, *name.encode()])
    worst = {}
    for key in G.LEAVES:
        bar = ("Q_bar" if full else "q_bar") if key == "q" else key + "_bar"
        if leaves[key] is None or not r[bar].any():
            continue
        x0 = leaves[key].numpy()
        for _ in range(N_DIRECTIONS):
            u = rng.standard_normal(x0.shape)
            if key == "q" and full:
                u = 0.5 * (u + u.transpose(0, 2, 1))
            elif key == "q":
                u[x0 == 0.0] = 0.0
            elif key == "P0":
                u = 0.5 * (u + u.T)
            elif key == "shift":
                u[0] = 0.0
            u /= np.sqrt((u * u).sum())
            fd, est = G.directional_derivative(c, 0, key, u)
            err = abs(fd - (r[bar] * u).sum()) / np.abs(r[bar]).max()
            worst[bar] = max(worst.get(bar, 0.0), err)
    print(name, " ".join(f"{key} {err:.2e}" for key, err in worst.items()))
    missed = {key: err for key, err in worst.items() if not err <= (FD_ROUNDING_BAR if (name, key) in FD_ROUNDING else FD_BAR)}
    assert worst and not missed, (name, missed)


def test_the_rounding_table_names_cases_and_blocks_that_exist():
    for (name, key), (cause, measured) in FD_ROUNDING.items():
        assert name in G.GRADIENT_CASES and key in _blocks(G.case(name)) and cause and FD_BAR < measured <= FD_ROUNDING_BAR


def test_all_filter_conventions_have_a_reference():
    """The 48 combinations of the device test: finite, and the second formulation agrees (the complete panel without the F jitter)."""
    c, full = K.case(K.CONVENTION_CASE), K.case(K.CONVENTION_CASE_COMPLETE)
    worst = 0.0
    for conv in K.CONVENTIONS:
        cc = c if conv["jitter_on_F"] else full
        a, b = G.logp_and_gradient(cc, 0, conv), G.logp_and_gradient(cc, 0, conv, lyapunov="doubling")
        for key in _blocks(cc):
            if key not in zero_blocks(cc):
                assert np.isfinite(a[key]).all() and np.abs(a[key]).max() > 0.0, (conv, key)
                worst = max(worst, np.abs(a[key] - b[key]).max() / np.abs(a[key]).max())
    print(f"conventions: kronecker against doubling {worst:.2e}")
    assert worst <= SECOND_BAR


def test_the_fused_chain_agrees_with_the_chain_on_its_own_T_and_R():
    """``fused_logp_and_gradient``: T_bar, R_bar and the filter's blocks are those of ``logp_and_gradient`` on the T, R it solved."""
    from geconpy_amd import workloads as wl

    nb, S = 2, 3
    sh = dict(zip(("n", "n_state", "n_lead", "k"), K.SC.SW17))
    b = wl.sw_shaped_batch(nb, **sh)
    pick = (np.arange(nb)[:, None] + np.arange(S)[None, :]) % nb
    c = K.build("sw17", nb=nb)
    fused = G.fused_logp_and_gradient(*(b[x][pick][0] for x in "ABCD"), c, 0)
    assert np.abs(fused["T"] - c["T"][0]).max() <= 1e-12
    plain = G.logp_and_gradient(dict(c, T=fused["T"][None], R=fused["R"][None]), 0)
    for key in _blocks(c):
        scale = np.abs(plain[key]).max()
        assert np.abs(fused[key] - plain[key]).max() <= 1e-12 * max(scale, 1.0), key
    assert all(np.abs(fused[key]).max() > 0.0 for key in ("A_bar", "B_bar", "C_bar", "D_bar"))


def test_no_new_kernel_uses_scratch_memory(tmp_path):
    import subprocess

    from geconpy_amd import build

    # the reverse sweep and R_bar / Q_bar in the gradient's unit, the storing forward pass in the unit the smoother launches it from
    found = {}
    for unit in ("launch_kalman_seg_grad.hip", "launch_kalman_seg_store.hip"):
        out = subprocess.run([build._hipcc(), *build.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "a.o"),
                              os.path.join(build.CSRC, unit)], cwd=build.CSRC, capture_output=True, text=True, check=True)
        names = re.findall(r"Function Name: (\S+)", out.stderr)
        sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
        assert len(names) == len(sizes)
        found[unit] = dict(zip(names, sizes))
    grad, store = found["launch_kalman_seg_grad.hip"], found["launch_kalman_seg_store.hip"]
    for kernel in ("kalman_seg_grad_kernel", "kseg_grad_rq_kernel"):
        assert [n for n in grad if kernel in n], (kernel, sorted(grad))
    assert [n for n in store if "kalman_seg_kernelILb1E" in n], sorted(store)
    assert not [n for n in grad if "kalman_seg_kernel" in n], sorted(grad)  # one kernel, compiled once
    assert all(size == "0" for unit in found.values() for size in unit.values()), found
