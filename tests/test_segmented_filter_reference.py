"""CPU: the numpy reference of the segmented filter (tests/segmented_filter_reference.py: oracle.kalman_filter_logp chained segment by
segment) against three other formulations of the same likelihood -- a time-varying loop written out directly, the log-density of the
stacked Gaussian the filter factorises (jitter off), and the oracle itself when all segments are identical.  Bars: 1e-10 relative
for the first two (two orders of summation of the same float64 recursion; the stacked form solves one (T_len p)-dimensional system of
condition <= 1e6 instead of T_len p-dimensional ones), exact for S = 1."""
import numpy as np
import pytest

import oracle

from tests import segmented_filter_cases as K
from tests.segmented_filter_reference import segment_of, segmented_filter

RTOL = 1e-10
LN2PI = np.log(2.0 * np.pi)


def _sym(A):
    return 0.5 * (A + A.T)


def _loop(y, segs, seg_start, a0, P0, shift, jitter=oracle.JITTER_DEFAULT, fill=oracle.MISSING_FILL):
    """The recursion of docs/design/segmented_filter.md written out with time-varying matrices (default conventions)."""
    n, m = y.shape[0], segs[0]["T"].shape[0]
    x0 = segs[0]
    a = np.zeros(m) if a0 is None else a0.copy()
    P = oracle.solve_discrete_lyapunov(x0["T"], x0["R"] @ x0["Q"] @ x0["R"].T) if P0 is None else P0.copy()
    ll = np.zeros(n)
    for t in range(n):
        x = segs[segment_of(seg_start, t)]
        p = x["Z"].shape[0]
        miss = np.isnan(y[t]) | (y[t] == fill)
        W = np.diag((~miss).astype(float))
        Zm, Hm = W @ x["Z"], W @ (np.zeros((p, p)) if x["H"] is None else x["H"])
        v = np.where(miss, 0.0, y[t]) - (np.zeros(p) if x["d"] is None else x["d"]) - Zm @ a
        F = Zm @ P @ Zm.T + Hm + jitter * np.eye(p)
        K_ = np.linalg.solve(F, Zm @ P).T
        a_f = a + K_ @ v
        I_KZ = np.eye(m) - K_ @ Zm
        P_f = _sym(I_KZ @ P @ I_KZ.T) + _sym(K_ @ Hm @ K_.T) + jitter * np.eye(m)
        if not miss.all():
            ll[t] = -0.5 * (p * LN2PI + np.linalg.slogdet(F)[1] + v @ np.linalg.solve(F, v))
        if t + 1 < n:
            s1 = segment_of(seg_start, t + 1)
            x1 = segs[s1]
            if shift is not None and t + 1 == seg_start[s1]:
                a_f = a_f + shift[s1]
            a = x1["T"] @ a_f
            P = _sym(x1["T"] @ P_f @ x1["T"].T) + _sym(x1["R"] @ x1["Q"] @ x1["R"].T)
    return ll, a_f, P_f


def _args(c, b):
    return (None if c["a0"] is None else c["a0"][b], None if c["P0"] is None else c["P0"][b],
            None if c["shift"] is None else c["shift"][b])


@pytest.mark.parametrize("name", K.ACCURACY_CASES)
def test_reference_equals_the_time_varying_loop(name):
    c = K.case(name)
    assert K.check_conditions(name) <= K.COND_MAX
    for b, ref in K.reference(name).items():
        ll, a_f, P_f = _loop(c["y"], K.draw(c, b), c["seg_start"], *_args(c, b))
        assert abs(ll.sum() - ref["logp"]) <= RTOL * abs(ref["logp"])
        assert np.abs(ll - ref["ll"]).max() <= RTOL * np.abs(ref["ll"]).max()
        assert np.abs(a_f - ref["a_last"]).max() <= RTOL * max(1.0, np.abs(ref["a_last"]).max())
        assert np.abs(P_f - ref["P_last"]).max() <= RTOL * np.abs(ref["P_last"]).max()


def _stacked_logpdf(y, segs, seg_start, a0, P0, shift):
    """log N(vec(y); mean, cov) of the whole panel (no missing entries, no jitter)."""
    n, m = y.shape[0], segs[0]["T"].shape[0]
    p = y.shape[1]
    x0 = segs[0]
    mu = [np.zeros(m) if a0 is None else a0]
    C = [[None] * n for _ in range(n)]
    C[0][0] = oracle.solve_discrete_lyapunov(x0["T"], x0["R"] @ x0["Q"] @ x0["R"].T) if P0 is None else P0
    for t in range(n - 1):
        s1 = segment_of(seg_start, t + 1)
        x1 = segs[s1]
        sh = shift[s1] if shift is not None and t + 1 == seg_start[s1] else 0.0
        mu.append(x1["T"] @ (mu[t] + sh))
        C[t + 1][t + 1] = x1["T"] @ C[t][t] @ x1["T"].T + x1["R"] @ x1["Q"] @ x1["R"].T
        for u in range(t + 1):
            C[t + 1][u] = x1["T"] @ C[t][u]
    mean = np.empty(n * p)
    cov = np.empty((n * p, n * p))
    for t in range(n):
        xt = segs[segment_of(seg_start, t)]
        mean[t * p:(t + 1) * p] = xt["Z"] @ mu[t] + (0.0 if xt["d"] is None else xt["d"])
        for u in range(t + 1):
            xu = segs[segment_of(seg_start, u)]
            blk = xt["Z"] @ C[t][u] @ xu["Z"].T
            if u == t and xt["H"] is not None:
                blk = blk + xt["H"]
            cov[t * p:(t + 1) * p, u * p:(u + 1) * p] = blk
            cov[u * p:(u + 1) * p, t * p:(t + 1) * p] = blk.T
    r = y.reshape(-1) - mean
    return -0.5 * (n * p * LN2PI + np.linalg.slogdet(cov)[1] + r @ np.linalg.solve(cov, r))


@pytest.mark.parametrize("builder", ("zc16", "dense33", "zc49", "dense64"))
@pytest.mark.parametrize("extras", ({}, dict(shift=True), dict(a0=True), dict(shift=True, a0=True, P0=True)))
def test_reference_equals_the_stacked_gaussian_density(builder, extras):
    c = K.build(builder, seg_start=(0, 1, 5), n=6, missing=(), **extras)
    cv = oracle.FilterConventions(jitter_on_F=False, jitter_on_P=False)
    for b in range(c["T"].shape[0]):
        a0, P0, shift = _args(c, b)
        ref = segmented_filter(c["y"], K.draw(c, b), c["seg_start"], a0=a0, P0=P0, shift=shift, conventions=cv)
        want = _stacked_logpdf(c["y"], K.draw(c, b), c["seg_start"], a0, P0, shift)
        assert abs(ref["logp"] - want) <= RTOL * abs(want)


@pytest.mark.parametrize("seg_start", ((0,), (0, 1), (0, 4), (0, 7), (0, 2, 3), tuple(range(8))))
def test_identical_segments_are_the_plain_filter(seg_start):
    c = SC_case()
    for b in range(c["T"].shape[0]):
        x = K.draw(c, b)[0]
        total, ll, stt = oracle.kalman_filter_logp(c["y"], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], return_states=True)
        ref = segmented_filter(c["y"], [x] * len(seg_start), seg_start)
        if len(seg_start) == 1:
            assert ref["logp"] == total and np.array_equal(ref["ll"], ll)
            assert np.array_equal(ref["a_last"], stt["a_filt"][-1]) and np.array_equal(ref["P_last"], stt["P_filt"][-1])
        else:
            assert abs(ref["logp"] - total) <= RTOL * abs(total)
            assert np.abs(ref["ll"] - ll).max() <= RTOL * np.abs(ll).max()
            assert np.abs(ref["P_last"] - stt["P_filt"][-1]).max() <= RTOL * np.abs(stt["P_filt"]).max()


def SC_case():
    return K.case("s1")


def test_shift_of_segment_zero_is_never_read():
    c = K.case("shift")
    sh = np.array(c["shift"][0])
    sh[0] = np.nan
    ref = segmented_filter(c["y"], K.draw(c, 0), c["seg_start"], shift=sh)
    assert ref["logp"] == K.reference("shift")[0]["logp"]
