"""GPU: ``dsge_spectral_moments_batched`` against the numpy reference (tests/spectral_moments_reference.py) on the cases of
tests/spectral_moments_cases.py.  Bar: 1e-9 of max|acov[0]| of the draw's reference for ``acov`` and of max_n |spectrum| for
``spectrum``, per output block, no floor at 1 -- the project's fixed bar for post-solve outputs."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from geconpy_amd import _lib, batched
from tests import spectral_moments_cases as cases

pytestmark = pytest.mark.gpu
BAR = 1e-9


def _kwargs(name, **over):
    kw = {**cases.case(name), **over}
    return (kw.pop("T"), kw.pop("R"), kw.pop("Q")), kw


@functools.lru_cache(maxsize=None)
def _result(name):
    args, kw = _kwargs(name)
    return batched.spectral_moments_batched(*args, **kw)


def _assert_parity(name, got, want):
    kw = cases.case(name)
    for b in range(cases.NB):
        if kw["acov"]:
            scale = np.abs(want["acov"][b, 0]).max()
            err = np.abs(got["acov"][b] - want["acov"][b]).max()
            print(f"{name} draw {b}: acov {err / scale:.2e} of max|acov[0]| = {scale:.3e}")
            assert err <= BAR * scale
        if kw["spectrum"]:
            scale = np.abs(want["spectrum"][b]).max()
            err = np.abs(got["spectrum"][b] - want["spectrum"][b]).max()
            print(f"{name} draw {b}: spectrum {err / scale:.2e} of max|spectrum| = {scale:.3e}")
            assert err <= BAR * scale


@pytest.mark.parametrize("name", cases.NAMES)
def test_parity_with_the_reference(name):
    want = cases.reference(name)
    assert want["cond"].max() <= cases.COND_BOUND
    got = _result(name)
    assert_array_equal(got["status"], 0)
    _assert_parity(name, got, want)


@pytest.mark.parametrize("name", ["sw17_band", "sw40_hp", "wide33_16"])
def test_two_calls_give_the_same_bits(name):
    args, kw = _kwargs(name)
    again = batched.spectral_moments_batched(*args, **kw)
    for key in ("acov", "spectrum"):
        if key in again and again[key] is not None:
            assert_array_equal(again[key], _result(name)[key])


@pytest.mark.parametrize("name", ["sw17_band", "sw16_hp"])
def test_device_tensors_on_a_side_stream_equal_the_host_twin(name):
    import torch
    from geconpy_amd.engine import LogpEngine

    eng = LogpEngine(0)
    dev = lambda a: None if a is None else eng.to_device(a)  # noqa: E731
    (T, R, Q), kw = _kwargs(name)
    kw.update(Z=dev(kw["Z"]), Hdiag=dev(kw["Hdiag"]), gain=dev(kw["gain"]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = eng.spectral_moments(dev(T), dev(R), dev(Q), **kw)
    side.synchronize()
    want = _result(name)
    assert_array_equal(got["acov"].cpu().numpy(), want["acov"])
    assert_array_equal(got["status"].cpu().numpy(), want["status"])
    if "spectrum" in want:
        assert_array_equal(got["spectrum"].cpu().numpy(), want["spectrum"])


def _doubled(name):
    """The case's three draws twice (six draws), gain None, the spectrum and the autocovariances both wanted."""
    (T, R, Q), kw = _kwargs(name, gain=None, spectrum=True, acov=True)
    rep = lambda a, batched_: a if a is None or not batched_ else np.concatenate([a, a])  # noqa: E731
    kw.update(Z=rep(kw["Z"], kw["Z"] is not None and kw["Z"].ndim == 3), Hdiag=rep(kw["Hdiag"], kw["Hdiag"] is not None and kw["Hdiag"].ndim == 2))
    return [np.concatenate([T, T]), np.concatenate([R, R]), rep(Q, kw["q_mode"].endswith("_batched"))], kw


def test_a_failed_and_a_singular_draw_and_chunking_leave_the_others_untouched():
    (T, R, Q), kw = _doubled("sw17_band")
    clean = batched.spectral_moments_batched(T, R, Q, **kw)
    assert_array_equal(clean["status"], 0)
    T = T.copy()
    T[3][:, 5] = 0.0
    T[3][5, 5] = 1.0  # an eigenvalue exactly 1: column 5 of I - T is exactly zero
    status = np.zeros(6, dtype=np.int32)
    status[1] = _lib.ST_NOT_CONVERGED
    dim, nf = clean["acov"].shape[-1], kw["n_grid"] // 2 + 1
    got = batched.spectral_moments_batched(T, R, Q, status=status, scratch_limit_bytes=2 * 16 * nf * dim * dim, **kw)
    assert got["status"].tolist() == [0, _lib.ST_NOT_CONVERGED, 0, _lib.ST_SPECTRAL_SINGULAR, 0, 0]
    for key in ("acov", "spectrum"):
        assert np.isnan(got[key][[1, 3]]).all()
        assert_array_equal(got[key][[0, 2, 4, 5]], clean[key][[0, 2, 4, 5]])
    # and the draws of the clean batch do not depend on the batch they are in
    assert_array_equal(clean["acov"][:3], clean["acov"][3:])
    assert_array_equal(clean["spectrum"][:3], clean["spectrum"][3:])


def test_hp_moments_of_a_unit_root_model_are_finite_and_its_unfiltered_ones_singular():
    name = "sw17_unit_root"
    got, want = _result(name), cases.reference(name)
    assert_array_equal(got["status"], 0)
    assert np.isfinite(got["acov"]).all()
    _assert_parity(name, got, want)
    args, kw = _kwargs(name, gain=None)
    got = batched.spectral_moments_batched(*args, **kw)
    assert_array_equal(got["status"], _lib.ST_SPECTRAL_SINGULAR)
    assert np.isnan(got["acov"]).all()


def test_frequencies_of_zero_gain_do_not_change_the_bits_whether_solved_or_not():
    args, kw = _kwargs("sw17_band", spectrum=False)
    assert (kw["gain"] == 0.0).sum() > 20
    got = batched.spectral_moments_batched(*args, **kw)
    assert_array_equal(got["acov"], _result("sw17_band")["acov"])
    assert_array_equal(got["status"], 0)


# ---- several frequencies per wavefront: the launcher makes ceil(32768 / batch) frequency groups, at most nf.  The cases above have
# 3 to 6 draws, hence one group per frequency.  1 200 draws of sw17_band (nf = 34) make 28 groups: the wavefronts of groups 0 .. 5
# solve two frequencies (n and n + 28), the others one.
REPS = 400


def _tiled(name, **over):
    (T, R, Q), kw = _kwargs(name, **over)
    rep = lambda a, batched_: a if a is None or not batched_ else np.tile(a, (REPS,) + (1,) * (a.ndim - 1))  # noqa: E731
    kw.update(Z=rep(kw["Z"], kw["Z"] is not None and kw["Z"].ndim == 3), Hdiag=rep(kw["Hdiag"], kw["Hdiag"] is not None and kw["Hdiag"].ndim == 2))
    T = np.tile(T, (REPS, 1, 1))
    for draw, root in ((10, 1.0), (11, -1.0)):  # an exact zero column of I - z T at w = 0 (n = 0) and at w = pi (n = 33 = 5 + 28)
        T[draw][:, 5] = 0.0
        T[draw][5, 5] = root
    status = np.zeros(3 * REPS, dtype=np.int32)
    status[7] = _lib.ST_NOT_CONVERGED
    return [T, np.tile(R, (REPS, 1, 1)), rep(Q, kw["q_mode"].endswith("_batched"))], dict(kw, status=status)


def _assert_tiled_equals_small(big, small, keys, odd):
    clean = np.setdiff1d(np.arange(3 * REPS), odd)
    for key in keys:
        assert_array_equal(big[key][clean], small[key][clean % 3])


def test_wavefronts_that_solve_two_frequencies_give_the_bits_of_one_frequency_each():
    """Band-pass gain, spectrum and autocovariances: every frequency is solved.  The draw with the root -1 turns singular in the
    SECOND frequency of its wavefront (n = 33 after n = 5), the one with the root 1 in the first (n = 0)."""
    args, kw = _tiled("sw17_band")
    assert 3 * REPS == 1200 and kw["n_grid"] // 2 + 1 == 34
    got = batched.spectral_moments_batched(*args, **kw)
    want = np.zeros(3 * REPS, dtype=np.int32)
    want[[7, 10, 11]] = _lib.ST_NOT_CONVERGED, _lib.ST_SPECTRAL_SINGULAR, _lib.ST_SPECTRAL_SINGULAR
    assert_array_equal(got["status"], want)
    for key in ("acov", "spectrum"):
        assert np.isnan(got[key][[7, 10, 11]]).all()
    _assert_tiled_equals_small(got, _result("sw17_band"), ("acov", "spectrum"), [7, 10, 11])


def test_two_frequencies_per_wavefront_with_unsolved_ones_between():
    """No spectrum: frequencies of zero gain are skipped.  Band-pass (n = 3 .. 11 solved: a solved frequency, then a skipped one) and
    a high-pass gain (n >= 20 solved: groups 0 .. 5 skip their first frequency and solve their second).  The roots 1 and -1 lie at
    frequencies of zero gain under the band-pass and are not reported; the high-pass solves n = 33 and reports the root -1."""
    small_args, small_kw = _kwargs("sw17_band", spectrum=False)
    high = (np.arange(34) >= 20).astype(np.float64)
    for gain, singular in ((small_kw["gain"], []), (high, [11])):
        args, kw = _tiled("sw17_band", spectrum=False, gain=gain)
        got = batched.spectral_moments_batched(*args, **kw)
        small = batched.spectral_moments_batched(*small_args, **dict(small_kw, gain=gain))
        assert_array_equal(small["status"], 0)
        want = np.zeros(3 * REPS, dtype=np.int32)
        want[7] = _lib.ST_NOT_CONVERGED
        want[singular] = _lib.ST_SPECTRAL_SINGULAR
        assert_array_equal(got["status"], want)
        assert np.isnan(got["acov"][[7] + singular]).all()
        assert np.isfinite(got["acov"][np.setdiff1d([10, 11], singular)]).all()
        _assert_tiled_equals_small(got, small, ("acov",), [7, 10, 11])
