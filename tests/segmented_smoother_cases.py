"""Inputs of the tests of the smoother across dated structural breaks (TEST INFRASTRUCTURE ONLY; a helper, not a test module): the
same arrays, built once and read-only, for tests/test_segmented_smoother_reference.py (the numpy forms against each other) and
tests/test_gpu_segmented_smoother.py (the device against the reference).

Every accuracy case of the segmented likelihood (tests/segmented_filter_cases.py: the zero-column and dense builders of
tests/smoother_cases.py at every edge of the LDS classes, every segment structure, input form and missing-data pattern) is one here,
plus the cases whose RANK differs between the segments of one draw: segment 1 has a shock without variance, segment 2 a T with one
more zero column -- at m = 17, m = 33 (the LDS images are re-staged) and m = 49 (the pointers switch).

``reference(name)`` -> draw -> dict(ll, a_pred, a_filt, P_pred, P_filt, smoothed_states, smoothed_covs, smoothed_shocks) from
``segmented_forward`` and ``segmented_rts_smoother`` (pinv form), computed once, shared, never modified."""
import functools

import numpy as np

import oracle

from tests import segmented_filter_cases as K
from tests.segmented_filter_reference import innovation_conditions
from tests.segmented_smoother_reference import segmented_forward, segmented_rts_smoother

RANK_CASES = {"ranks_m17": "sw17", "ranks_m33": "zc33", "ranks_m49": "zc49"}
ACCURACY_CASES = K.ACCURACY_CASES + tuple(RANK_CASES)
KEYS = ("ll", "a_pred", "a_filt", "P_pred", "P_filt", "smoothed_states", "smoothed_covs", "smoothed_shocks")
ZERO_SHOCK = (1, 1)  # (segment, shock)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _rank_case(builder):
    c = dict(K.build(builder, zero_shock=ZERO_SHOCK))
    T = np.array(c["T"])
    for b in range(T.shape[0]):  # segment 2: the first column of T that is not zero becomes one
        T[b, 2][:, np.flatnonzero(np.abs(T[b, 2]).sum(axis=0) > 0)[0]] = 0.0
    c["T"] = T
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def case(name):
    return _rank_case(RANK_CASES[name]) if name in RANK_CASES else K.case(name)


def reference_of(c, conventions=None):
    cv = None if conventions is None else oracle.FilterConventions(**conventions)
    out = {}
    for b in range(c["T"].shape[0]):
        segs = K.draw(c, b)
        fwd = segmented_forward(c["y"], segs, c["seg_start"], a0=None if c["a0"] is None else c["a0"][b],
                                P0=None if c["P0"] is None else c["P0"][b], shift=None if c["shift"] is None else c["shift"][b],
                                conventions=cv)
        a_s, V, eps = segmented_rts_smoother(fwd, segs, c["seg_start"])
        out[b] = dict(fwd, smoothed_states=a_s, smoothed_covs=V, smoothed_shocks=eps)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(case(name))


def scales(c, b, ref):
    """The scale of each block of the 1e-9 bar: the largest filtered mean, the largest predicted covariance, the largest shock
    standard deviation of the draw's segments (what tests/smoother_cases.py takes, without its floor of 1 on the means)."""
    return (np.abs(ref["a_filt"]).max(), np.abs(ref["P_pred"]).max(), max(np.sqrt(np.diag(x["Q"]).max()) for x in K.draw(c, b)))


def check_conditions(name):
    """From the reference alone: finite ll and cond_2(F_t) <= K.COND_MAX at every period of every draw.  Returns the largest cond."""
    c, worst = case(name), 0.0
    for b, ref in reference(name).items():
        assert np.isfinite(ref["ll"]).all(), (name, b)
        worst = max(worst, innovation_conditions(c["y"], K.draw(c, b), c["seg_start"], ref).max())
    assert worst <= K.COND_MAX, (name, worst)
    return worst
